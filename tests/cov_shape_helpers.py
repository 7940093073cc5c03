"""Shared by tests/test_host_cov_shapes.py and tests/test_gpu_cov_shapes.py: the graphs at which the eight covariance kernels
(csrc/pps_cov.hip, csrc/pps_cov_dense.hip, csrc/pps_cov_wide.hip) are pinned, the front shapes each graph exists for, the node pairs
pps_cov_access must answer, and a reference that is better than what it measures.  Nothing in here is code under test.

  TABLE / BAND / DENSE   small graphs of linsolve_helpers.loop_graph (and one of synth.small_world), each with the contract LINES it is
                         in the table for.  A line is a predicate over pps_analysis_dump alone (front_facts) with one assert message;
                         assert_entry runs the lines of one entry, so that a change of the ordering cannot silently empty a test.
                         Band entries (max front <= 127 rows, at most ~250 scalars) run k_cov_level, k_cov_path / k_cov_gram, and the
                         dense-front pass forced onto them; dense entries (at most 600 scalars) run the dense-front pass and the wide walk.
  BAND_LINES             what k_cov_level and cov_walk branch on: the dynamic-LDS ceiling beyond 64 KB (p = 48, b >= 75), b * b and b * p
                         against one pass of 256 threads, p * p <= 256 and beyond, b > 64 in the row loop of the walk, p = 3 / 6 / odd / 48,
                         a one-front graph, a level of three fronts, nodes off the first pivot of their front and at its end.
  DENSE_LINES            the tile edges of k_cov_dense_pre / gather / sba / saa: nt = ceil(p / 16) in 1 .. 4 with full and partial last
                         tiles, k-slabs of 32 (b % 32 in {0, 1, >= 30}, b < 32), 64-row strips whose last one leaves waves 1 .. 3 without a
                         row, the second 256-row slab of G, a child map that is not contiguous in its parent.
                         Every shape of a graph is a multiple of 3 (poses 6, planes 3), so p = 64 -- four full tiles -- cannot occur
                         through a graph, and neither can p = 16, 17, 32, 33 or b = 31, 32, 64, 65, 80: the stand-alone program of
                         tests/cpp/cov_dense_emu.cpp runs chains of those shapes (p = 64 with b = 256 and 257; p in {16, 17, 32, 33} with
                         b in {31, 32, 33, 64, 65, 80}; p = 1 with b = 1) against its sequential restatement.
  role_nodes             about a dozen nodes by role, for pps_cov_block: off the first pivot (a plane and a pose), ending a front, in the
                         root front, the deepest leaf, two in diverging subtrees, a front / ancestor pair
  pattern_pairs          every ordered pair of distinct nodes that share a front as (pivot, row) -- the pairs pps_cov_access answers --
                         and the subset that no factor joins: the fill of the factor, which the older tests never read
  longdouble_inverse     column Cholesky and triangular inverse in np.longdouble (64-bit mantissa): 2.6e-19 from a 40-digit inverse where
                         np.linalg.inv sits at 3.8e-16, so that d = |np.linalg.inv - reference| measures the float64 inverse, not the reference
  block_errors           e and d over a list of blocks: the measure of cov_block_helpers.block_err against the reference's diagonal blocks
"""
import numpy as np

from cov_block_helpers import block_err, common_suffix
from cov_factor_helpers import node_paths, rows_of
from cov_helpers import factor_pairs
from linsolve_helpers import front_shapes, loop_graph
from pop_up_slam_amd import synth


# ---- facts of an analysis ----------------------------------------------------------------------------------------------------
def front_facts(A, lay, sel=None):
    """what the contract lines look at, from the analysis dump alone"""
    info = node_paths(A, lay)
    fr = front_shapes(A)
    noncontig = False
    for s, (p, b) in enumerate(fr):
        cm = np.asarray(A["cmap"][A["f_cmap_off"][s]:A["f_cmap_off"][s] + b])
        if b and not np.array_equal(cm, np.arange(cm[0], cm[0] + b)):
            noncontig = True
    sel = role_nodes(A, lay) if sel is None else sel
    return {
        "fronts": fr,
        "with_b": [(p, b) for p, b in fr if b > 0],
        "max_front": int(A["max_front"]),
        "n_scalars": int(A["n_scalars"]),
        "widest_level": int(np.max(np.diff(np.asarray(A["level_off"])))),
        # (dim, first local pivot, pivots of the front) of every node
        "nodes": [(lay[n][1], info[n][1], int(A["f_p"][info[n][0]])) for n in sorted(lay)],
        "walk_b": sorted({int(A["f_b"][s]) for n in sel for s in info[n][2]}),
        "noncontiguous_cmap": noncontig,
    }


# one line: name -> (predicate over front_facts, what is missing when it fails)
BAND_LINES = {
    "lds_beyond_64k": (lambda f: any((2 * p * p + b * p + 2) * 8 > 65536 for p, b in f["fronts"]),
                       "no front whose k_cov_level needs more than 64 KB of dynamic LDS (p = 48 and b >= 75)"),
    "narrow_tall": (lambda f: any(p <= 6 and b >= 100 for p, b in f["fronts"]), "no front with p <= 6 and b >= 100 (b * b far beyond one pass, b * p just beyond)"),
    "walk_b_beyond_64": (lambda f: any(b > 64 for b in f["walk_b"]), "no front with b > 64 on the root path of a queried node (second round of cov_walk's row loop)"),
    "pp_within_one_pass": (lambda f: any(p * p <= 256 for p, _ in f["fronts"]), "no front with p * p <= 256"),
    "pp_beyond_one_pass": (lambda f: any(p * p > 256 for p, _ in f["fronts"]), "no front with p * p > 256"),
    "bp_within_one_pass": (lambda f: any(b * p <= 256 for p, b in f["with_b"]), "no front with 0 < b * p <= 256"),
    "p3": (lambda f: any(p == 3 for p, _ in f["fronts"]), "no front with p = 3"),
    "p6": (lambda f: any(p == 6 for p, _ in f["fronts"]), "no front with p = 6"),
    "p_odd": (lambda f: any(p % 2 == 1 and p > 3 for p, _ in f["fronts"]), "no front whose p is an odd multiple of 3 beyond 3"),
    "p48": (lambda f: any(p == 48 for p, _ in f["fronts"]), "no front with p = 48"),
    "one_front": (lambda f: len(f["fronts"]) == 1 and f["fronts"][0][1] == 0, "not a one-front graph"),
    "level_of_three": (lambda f: f["widest_level"] >= 3, "no level with three fronts (k_cov_level with more than two workgroups)"),
    "plane_off_first_pivot": (lambda f: any(d == 3 and m0 > 0 for d, m0, _ in f["nodes"]), "no plane whose first pivot is not the first of its front"),
    "pose_off_first_pivot": (lambda f: any(d == 6 and m0 > 0 for d, m0, _ in f["nodes"]), "no pose whose first pivot is not the first of its front"),
    "ends_its_front": (lambda f: any(m0 > 0 and m0 + d == p for d, m0, p in f["nodes"]), "no node that follows another in its front and ends it (m0 + D == p)"),
}


def _tiles(p):
    return (p + 15) // 16


DENSE_LINES = {
    **{f"nt{k}_partial": (lambda f, k=k: any(_tiles(p) == k and p % 16 for p, _ in f["with_b"]), f"no front with b > 0, {k} column tiles and a partial last tile")
       for k in (1, 2, 3, 4)},
    "p48_full_tile": (lambda f: any(p == 48 for p, _ in f["with_b"]), "no front with b > 0 and p = 48 (nt = 3, the last tile full)"),
    "b_below_one_slab": (lambda f: any(b < 32 for _, b in f["with_b"]), "no front with 0 < b < 32"),
    "b_mod32_0": (lambda f: any(b % 32 == 0 for _, b in f["with_b"]), "no front with b % 32 == 0"),
    "b_mod32_1": (lambda f: any(b % 32 == 1 for _, b in f["with_b"]), "no front with b % 32 == 1 (one row in the last k-slab)"),
    "b_mod32_30": (lambda f: any(b % 32 >= 30 for _, b in f["with_b"]), "no front with b % 32 >= 30"),
    "last_strip_one_wave": (lambda f: any(b > 64 and 0 < b % 64 <= 16 for _, b in f["with_b"]),
                            "no front of more than one strip with 0 < b % 64 <= 16 (waves 1 .. 3 of the last strip own no row)"),
    "g_second_slab": (lambda f: any(b > 256 for _, b in f["with_b"]), "no front with b > 256 (second 256-row slab of k_cov_dense_pre)"),
    "g_first_slab_only": (lambda f: any(b <= 256 for _, b in f["with_b"]), "no front with 0 < b <= 256"),
    "noncontiguous_cmap": (lambda f: f["noncontiguous_cmap"], "no child whose cmap is not contiguous in its parent"),
}
# (nt = 1, 2, 3, 4 on a front with b > 0: implied by the four partial lines, which are all reachable; p = 48 is the one full last tile a graph can have)


# ---- the table ---------------------------------------------------------------------------------------------------------------
# name: (maker, "band" | "dense", band lines it is in the table for, dense lines it is in the table for).  Searched on the CPU over
# loop_graph(n_poses, loops, n_planes, seen, seed) and synth.small_world: per line the smallest graph found that meets it.
TABLE = {}


def _entry(name, make, kind, band=(), dense=()):
    assert all(l in BAND_LINES for l in band) and all(l in DENSE_LINES for l in dense)
    TABLE[name] = (make, kind, tuple(band), tuple(dense))


_entry("loop_2p", lambda: loop_graph(2, 0), "band", band=("one_front", "pp_within_one_pass", "pose_off_first_pivot", "ends_its_front"))
_entry("small_world_5_3", lambda: synth.small_world(5, 3), "band", band=("p_odd", "bp_within_one_pass"), dense=("nt1_partial", "b_below_one_slab"))
_entry("loop_6p_4x3", lambda: loop_graph(6, 0, 4, 3), "band", band=("bp_within_one_pass", "p_odd", "plane_off_first_pivot", "pp_beyond_one_pass"),
       dense=("nt1_partial", "nt2_partial", "b_below_one_slab", "g_first_slab_only"))
_entry("loop_20p_40l_10x5", lambda: loop_graph(20, 40, 10, 5), "band", band=("level_of_three", "p6", "p_odd", "plane_off_first_pivot", "walk_b_beyond_64"),
       dense=("nt3_partial", "b_mod32_0", "b_mod32_1", "last_strip_one_wave", "noncontiguous_cmap"))
_entry("loop_20p_200l_10x5_s2", lambda: loop_graph(20, 200, 10, 5, seed=2), "band", band=("p3", "p48", "level_of_three"), dense=("p48_full_tile", "b_mod32_30"))
_entry("loop_30p_200l", lambda: loop_graph(30, 200), "band",
       band=("lds_beyond_64k", "narrow_tall", "walk_b_beyond_64", "p48", "p6", "level_of_three", "pose_off_first_pivot", "ends_its_front"),
       dense=("p48_full_tile", "b_mod32_30", "last_strip_one_wave", "noncontiguous_cmap"))
_entry("dense_24p_400l_8x6", lambda: loop_graph(24, 400, 8, 6), "dense", dense=("nt4_partial", "nt2_partial", "noncontiguous_cmap"))
_entry("dense_72p_400l_8x6", lambda: loop_graph(72, 400, 8, 6), "dense", dense=("g_second_slab", "g_first_slab_only", "nt4_partial", "b_mod32_0", "last_strip_one_wave"))
BAND = [n for n in TABLE if TABLE[n][1] == "band"]
DENSE = [n for n in TABLE if TABLE[n][1] == "dense"]


def entry_lines(name):
    return TABLE[name][2], TABLE[name][3]


def analysed(name):
    """(graph handle, spec, analysis dump, node layout) of a table entry, analysed in analytic-Jacobian mode like the GPU test builds it"""
    import pop_up_slam_amd as P
    from linsolve_helpers import spec_layout
    spec = TABLE[name][0]()
    g = P.Graph(jacobian_mode=1); spec.replay(g); g.analyze()
    A = g.analysis_dump()
    return g, spec, A, spec_layout(spec, A)


def assert_entry(name, A, lay, spec):
    """the contract of one entry; returns (front facts, role nodes, pattern pairs, pairs no factor joins)"""
    _, kind, band, dense = TABLE[name]
    sel = role_nodes(A, lay)
    f = front_facts(A, lay, sel)
    if kind == "band":
        assert f["max_front"] <= 127, (name, "not a band graph", f["max_front"])
        assert f["n_scalars"] <= 252, (name, "band entries stay within ~250 scalars", f["n_scalars"])
    else:
        assert f["max_front"] > 127, (name, "not a dense-front graph", f["max_front"])
        assert f["n_scalars"] <= 600, (name, "dense entries stay within 600 scalars", f["n_scalars"])
    assert max(p for p, _ in f["fronts"]) <= (48 if kind == "band" else 64), (name, f["fronts"])
    for line in band:
        assert BAND_LINES[line][0](f), (name, line, BAND_LINES[line][1], f["fronts"])
    for line in dense:
        assert DENSE_LINES[line][0](f), (name, line, DENSE_LINES[line][1], f["fronts"])
    pairs, fill = pattern_pairs(A, lay, factor_pairs([(int(a), int(b)) for a, b in spec.f_nodes]))
    if len(f["fronts"]) > 1:
        assert fill, (name, "every pair of the pattern is joined by a factor: no fill to compare")
    return f, sel, pairs, fill


def uncovered_lines():
    """the lines no entry claims (the union contract: must be empty)"""
    band = set().union(*[set(TABLE[n][2]) for n in TABLE if TABLE[n][1] == "band"])
    dense = set().union(*[set(TABLE[n][3]) for n in TABLE])
    return sorted(set(BAND_LINES) - band), sorted(set(DENSE_LINES) - dense)


# ---- nodes and pairs ---------------------------------------------------------------------------------------------------------
def role_nodes(A, lay):
    """about a dozen nodes by role (every role the tree has; a one-front graph has few), in a fixed order without repeats"""
    info = node_paths(A, lay)
    ids = sorted(lay)
    F = int(A["n_fronts"])
    first = lambda it: next(iter(it), None)
    widest = max(range(F), key=lambda s: rows_of(A, s))
    deep = max(ids, key=lambda n: len(info[n][2]))
    root = [s for s in range(F) if int(A["f_b"][s]) == 0][-1]
    tall = max(range(F), key=lambda s: int(A["f_b"][s]))
    pick = [
        first(n for n in ids if lay[n][1] == 3 and info[n][1] > 0),                                   # a plane off the first pivot
        first(n for n in ids if lay[n][1] == 6 and info[n][1] > 0),                                   # a pose off the first pivot
        first(n for n in ids if info[n][1] > 0 and info[n][1] + lay[n][1] == int(A["f_p"][info[n][0]])),      # ends its front
        first(n for n in ids if info[n][0] == root),                                                  # in the root front
        deep,                                                                                         # the deepest leaf
        first(n for n in ids if info[n][0] not in info[deep][2] and info[deep][0] not in info[n][2]),  # in a subtree that diverges from it
        first(n for n in ids if info[n][0] != info[deep][0] and info[n][0] in info[deep][2][1:-1]),    # in an ancestor of it below the root
        first(n for n in ids if info[n][0] == widest),
        first(n for n in ids if info[n][0] == tall),                                                  # the front with the most rows below its pivots
        first(n for n in reversed(ids) if lay[n][1] == 3),
        ids[0], ids[len(ids) // 2], ids[-1],
    ]
    return list(dict.fromkeys(int(n) for n in pick if n is not None))


def roles_present(A, lay, sel):
    """what a node set exercises in pps_cov_block, as booleans"""
    info = node_paths(A, lay)
    pairs = [(a, b) for i, a in enumerate(sel) for b in sel[i + 1:]]
    plen = lambda n: sum(int(A["f_p"][s]) for s in info[n][2])
    return {
        "off_first_pivot": any(info[n][1] > 0 for n in sel),
        "root": any(int(A["f_b"][info[n][0]]) == 0 for n in sel),
        "diverge": any(common_suffix(A, info[a][2], info[b][2]) < min(plen(a), plen(b)) for a, b in pairs),
        "ancestor": any(info[a][0] != info[b][0] and (info[a][0] in info[b][2] or info[b][0] in info[a][2]) for a, b in pairs),
    }


def front_nodes(A, lay, s):
    """(nodes whose scalars are pivots of front s, nodes with rows below them), each in row order"""
    at = {lay[n][0]: n for n in lay}
    po, p = int(A["f_poff"][s]), int(A["f_p"][s])
    piv = [at[int(v)] for v in A["pidx"][po:po + p] if int(v) in at]
    bnd = [at[int(v)] for v in A["bidx"][A["f_bidx_off"][s]:A["f_bidx_off"][s + 1]] if int(v) in at]
    return piv, bnd


def pattern_pairs(A, lay, joined=()):
    """(pairs, fill): every ordered pair (r, c), r != c, with one node a pivot of a front the other has rows in -- what pps_cov_access must
    answer, from the dump alone -- and those of them that no factor of `joined` (unordered node pairs) joins"""
    out = set()
    for s in range(int(A["n_fronts"])):
        piv, bnd = front_nodes(A, lay, s)
        for a in piv:
            for b in piv + bnd:
                if a != b:
                    out.add((a, b)); out.add((b, a))
    joined = {(a, b) for a, b in joined} | {(b, a) for a, b in joined}
    pairs = sorted(out)
    return pairs, [q for q in pairs if q not in joined]


# ---- reference ---------------------------------------------------------------------------------------------------------------
def have_long_double():
    return np.finfo(np.longdouble).nmant >= 63


def longdouble_inverse(H):
    """H^-1 of a symmetric positive definite H in np.longdouble: column Cholesky, the inverse of the triangle row by row, X' X.  Where
    long double is no wider than double, the float64 inverse of cov_helpers.cpu_inverses (and a printed note that the old yardstick is in use)."""
    if not have_long_double():
        from cov_helpers import cpu_inverses
        print("cov_shape_helpers: np.longdouble has no 64-bit mantissa here -- the old yardstick (two float64 inverses) is in use")
        return cpu_inverses(np.asarray(H, dtype=np.float64))[1]
    M = np.asarray(H, dtype=np.longdouble)
    n = len(M)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = M[j:, j] - L[j:, :j] @ L[j, :j]
        assert v[0] > 0, "not positive definite"
        L[j:, j] = v / np.sqrt(v[0])
    X = np.zeros((n, n), dtype=np.longdouble)                # X = L^-1, row i from the rows above it
    for i in range(n):
        r = -(L[i, :i] @ X[:i, :])
        r[i] += 1
        X[i] = r / L[i, i]
    return X.T @ X


def block_errors(blocks, Sref, S1, span):
    """blocks: [(r, c, M)], M = Sigma(node r, node c) as delivered.  Returns (e, d): the worst block_err of M and of S1's block against Sref,
    both normalised by sqrt(|Sref(r, r)|_F |Sref(c, c)|_F)"""
    e = d = 0.0
    for r, c, M in blocks:
        sr, sc = span(r), span(c)
        eb = block_err(M, Sref[sr, sc], Sref[sr, sr], Sref[sc, sc])
        e = eb if not eb <= e else e                         # (a NaN block is the worst block)
        d = max(d, block_err(S1[sr, sc], Sref[sr, sc], Sref[sr, sr], Sref[sc, sc]))
    return float(e), float(d)


def split_joint(M, nodes, lay):
    """the blocks [(r, c, M_rc)] of a joint or rows x cols matrix over `nodes` x `nodes`"""
    return split_block(M, nodes, nodes, lay)


def split_block(M, rows, cols, lay):
    ro = np.concatenate([[0], np.cumsum([lay[n][1] for n in rows])]); co = np.concatenate([[0], np.cumsum([lay[n][1] for n in cols])])
    assert M.shape == (ro[-1], co[-1])
    return [(r, c, M[ro[i]:ro[i + 1], co[j]:co[j + 1]]) for i, r in enumerate(rows) for j, c in enumerate(cols)]
