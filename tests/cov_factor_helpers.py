"""Shared by tests/test_host_cov_factor.py and tests/test_gpu_cov_factor.py: graphs, node sets and their shape contract.

  GRAPHS            the four dense cases of tests/linsolve_helpers.py, and a fifth of the same maker (300 poses, 3 000 loop closures: a front
                    of 1 290 rows): none of the four (max front 162 .. 300 rows) nor the first 1 400 lines of sphere2500 (252) passes 1 024
  choose_nodes      about 12 nodes of a graph, from the analysis dump alone: through the widest front, in the root front, off the first
                    pivot of their front, in diverging subtrees, in a front and in one of its ancestors, planes where the graph has them
  contract          what a node set exercises, as booleans; the CPU test asserts them, so that a change of the ordering cannot empty a test
"""
import numpy as np

from cov_block_helpers import common_suffix, elimination_positions, node_front, path_to_root
from linsolve_helpers import CASES, loop_graph

DENSE = ["dense_48p_150l_10x5", "dense_64p_200l", "dense_100p_400l", "dense_100p_100l_30x8"]
WIDE = "dense_300p_3000l"
GRAPHS = {**{name: CASES[name][0] for name in DENSE}, WIDE: lambda: loop_graph(300, 3000, seed=2)}
# rows (p + b) the widest front on the paths of the chosen nodes must exceed, per graph
MIN_ROWS = {"dense_48p_150l_10x5": 127, "dense_64p_200l": 127, "dense_100p_400l": 256, "dense_100p_100l_30x8": 127, WIDE: 1024, "sphere2500_1400": 127}


def node_paths(A, lay):
    """node id -> (front, local index of its first pivot, path of fronts leaf -> root)"""
    _, epos = elimination_positions(A)
    out = {}
    for n in sorted(lay):
        s, local = node_front(A, epos, lay[n][0])
        out[n] = (s, local, path_to_root(A, s))
    return out


def rows_of(A, s):
    return int(A["f_p"][s]) + int(A["f_b"][s])


def choose_nodes(A, lay, n_spread=6):
    info = node_paths(A, lay)
    ids = sorted(lay)
    widest = max(range(A["n_fronts"]), key=lambda s: rows_of(A, s))
    through = [n for n in ids if widest in info[n][2]]
    pick = [max(through, key=lambda n: len(info[n][2]))]                        # the longest walk through the widest front
    root = [s for s in range(A["n_fronts"]) if int(A["f_b"][s]) == 0][-1]
    pick.append(next(n for n in ids if info[n][0] == root))
    pick.append(next(n for n in ids if info[n][1] != 0))
    deep = max(ids, key=lambda n: len(info[n][2]))                              # a leaf-most node and one in the middle of its path
    mid = info[deep][2][len(info[deep][2]) // 2]
    pick += [deep, next(n for n in ids if info[n][0] == mid)]
    pick.append(next(n for n in ids if info[n][0] not in info[deep][2] and info[deep][0] not in info[n][2]))      # outside that path
    planes = [n for n in ids if lay[n][1] == 3]
    pick += [planes[k] for k in sorted(set(np.linspace(0, len(planes) - 1, 3).astype(int).tolist()))] if planes else []
    pick += [ids[k] for k in sorted(set(np.linspace(0, len(ids) - 1, n_spread).astype(int).tolist()))]
    return list(dict.fromkeys(int(n) for n in pick))


def contract(A, lay, sel):
    info = node_paths(A, lay)
    paths = [info[n][2] for n in sel]
    rows = max(rows_of(A, s) for p in paths for s in p)
    pairs = [(a, b) for i, a in enumerate(sel) for b in sel[i + 1:]]
    return {
        "rows": rows,
        "root_b0": any(int(A["f_b"][p[-1]]) == 0 and info[n][0] == p[-1] for n, p in zip(sel, paths)),
        "off_first_pivot": any(info[n][1] != 0 for n in sel),
        "diverge": any(common_suffix(A, info[a][2], info[b][2]) < min(sum(int(A["f_p"][s]) for s in info[a][2]), sum(int(A["f_p"][s]) for s in info[b][2]))
                       for a, b in pairs),
        "ancestor": any(info[a][0] != info[b][0] and (info[a][0] in info[b][2] or info[b][0] in info[a][2]) for a, b in pairs),
    }


def assert_contract(name, A, lay, sel):
    c = contract(A, lay, sel)
    assert c["rows"] > MIN_ROWS[name], (name, c)
    assert c["root_b0"] and c["off_first_pivot"] and c["diverge"] and c["ancestor"], (name, c)
    return c
