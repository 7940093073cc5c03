"""CPU: the launch schedule of K3 as a value (csrc/pps_k3_plan.h), compiled with g++ alone (tests/cpp/k3_plan_host.cpp) and driven by the
arrays of pps_analysis_dump.  The whole K3Plan of every case is compared with tests/golden/k3_plan.json -- what the commit before the plan
existed decided for the same graphs (the file's header says how it was recorded) --, every case is shown to take the branch it is here
for, and the two formulas the header merged are held against transcriptions of the expressions they replaced."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import pop_up_slam_amd as P
from linsolve_helpers import loop_graph
from pop_up_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip = C.POINTER(C.c_int)
SW_NAMES = ("no_preassemble", "no_solve_flow", "no_root_fuse", "no_strip", "trace")

GRAPHS = {
    "a_corridor150": lambda: synth.corridor(150, 32, seed=8),                       # whole tree in two launches
    "b_corridor2000": lambda: synth.corridor(2000, 400, seed=42),                   # > 100 groups: a launch per stage, fused root
    "c_fronts_65_80": lambda: synth.corridor(400, 40, obs_per_pose=13, seed=5),     # test_gpu_solve.py::test_fronts_of_65_to_80_rows
    "d_loops_64_200": lambda: loop_graph(64, 200),                                  # loop closures: dense fronts
    "e_one_pose": lambda: synth.small_world(1, 3, seed=4),
    "e_small5": lambda: synth.small_world(5, 3, seed=1),
}
# case -> (graph, switches)
CASES = {k: (k, {}) for k in GRAPHS}
CASES.update({
    "f_a_no_preassemble": ("a_corridor150", {"no_preassemble": 1}),
    "f_a_no_solve_flow": ("a_corridor150", {"no_solve_flow": 1}),
    "f_a_no_root_fuse": ("a_corridor150", {"no_root_fuse": 1}),
    "f_a_plain_schedule": ("a_corridor150", {"no_preassemble": 1, "no_solve_flow": 1, "no_root_fuse": 1}),
    "f_c_no_strip": ("c_fronts_65_80", {"no_strip": 1}),
})


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("k3_plan") / "libk3plan.so"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "pop_up_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "k3_plan_host.cpp"), "-o", str(so)])
    L = C.CDLL(str(so))
    L.k3_plan_json.restype = C.c_int
    L.k3_plan_json.argtypes = [_ip] * 14 + [C.c_char_p, C.c_int]
    L.k3_flow_waves.restype = C.c_int
    L.k3_flow_waves.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_longlong]
    L.k3_flow_fixed_bytes.restype = C.c_longlong; L.k3_flow_fixed_bytes.argtypes = [C.c_int]
    L.k3_solve_lds_bytes.restype = C.c_longlong; L.k3_solve_lds_bytes.argtypes = [C.c_int]
    L.k3_group_fits_pre.restype = C.c_int; L.k3_group_fits_pre.argtypes = [_ip, _ip, C.c_int, C.c_int]
    L.k3_const.restype = C.c_longlong; L.k3_const.argtypes = [C.c_int]
    return L


@pytest.fixture(scope="module")
def dumps(built):
    """analysis only (no device): the dump of every graph, once"""
    out = {}
    for name, mk in GRAPHS.items():
        g = P.Graph(); mk().replay(g); g.analyze()
        out[name] = g.analysis_dump()
        g.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "k3_plan.json")) as f:
        return json.load(f)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def front_stage(A):
    """stage of every front, by group membership (glvl_fronts lists the fronts group by group, the groups stage by stage)"""
    st = np.zeros(A["n_fronts"], dtype=np.int64)
    for s in range(A["n_stages"]):
        for gi in range(A["stage_grp_off"][s], A["stage_grp_off"][s + 1]):
            a, b = A["glvl_front_off"][A["grp_lvl_off"][gi]], A["glvl_front_off"][A["grp_lvl_off"][gi + 1]]
            st[A["glvl_fronts"][a:b]] = s
    return st


def band_levels(A):
    """levels per band: not in the dump -- the one figure with stage == f_level // band_levels for every front"""
    st = front_stage(A)
    fits = [bn for bn in range(1, max(2, A["n_levels"] + 1)) if np.array_equal(A["f_level"] // bn, st)]
    assert fits, "no band depth explains the stages"
    return fits[0]


def plan_of(lib, A, sw):
    counts = _i32([A["n_stages"], A["n_groups"], A["n_levels"], A["n_fronts"], band_levels(A)])
    arrs = [_i32(A[k]) for k in ("stage_grp_off", "grp_lvl_off", "glvl_front_off", "glvl_fronts", "stage_max_front", "stage_max_width", "f_p", "f_b",
                                 "f_level", "level_off", "level_fronts", "f_el_off")]
    swv = _i32([int(sw.get(k, 0)) for k in SW_NAMES])
    buf = C.create_string_buffer(1 << 20)
    n = lib.k3_plan_json(counts.ctypes.data_as(_ip), *[a.ctypes.data_as(_ip) for a in arrs], swv.ctypes.data_as(_ip), buf, len(buf))
    assert 0 < n < len(buf)
    return json.loads(buf.value.decode())


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_equals_the_recorded_schedule(lib, dumps, golden, case):
    graph, sw = CASES[case]
    assert plan_of(lib, dumps[graph], sw) == golden["cases"][case]


def test_every_case_takes_its_branch(lib, dumps):
    plan = {c: plan_of(lib, dumps[g], sw) for c, (g, sw) in CASES.items()}
    a = plan["a_corridor150"]
    assert a["form"] == "band_all" and len(a["stages"]) >= 2 and a["all"]["n_groups"] == dumps["a_corridor150"]["n_groups"] <= 100
    assert all(s["pre"] and s["reg_only"] for s in a["stages"]) and a["all"]["nw_solve"] >= min(8, a["all"]["max_grp_fronts"])
    b = plan["b_corridor2000"]
    assert b["form"] == "band_stages" and dumps["b_corridor2000"]["n_groups"] > 100 and b["all"]["n_groups"] == 0
    assert any(s["pre"] for s in b["stages"]) and b["root"]["fusable"] and b["stages"][-1]["grp_count"] == 1
    c = plan["c_fronts_65_80"]
    assert c["form"] == "band_stages" and any(s["r5_ok"] and not s["reg_only"] and not s["pre"] for s in c["stages"])
    assert all(s["nw_factor_r5"] <= 4 and s["lds_factor_r5"] == 8 * s["pw_factor_gen"] * s["nw_factor_r5"] for s in c["stages"])
    assert not any(s["r5_ok"] for s in plan["f_c_no_strip"]["stages"])
    d = plan["d_loops_64_200"]
    assert d["form"] == "dense" and len(d["dw_asm"]) == dumps["d_loops_64_200"]["n_fronts"] + dumps["d_loops_64_200"]["n_levels"]
    # a single stage never takes the whole-tree form; its one group is the fused root launch -- one front: barrier walk, small5's three: data flow
    for e in ("e_one_pose", "e_small5"):
        assert plan[e]["form"] == "band_stages" and len(plan[e]["stages"]) == 1 and plan[e]["root"]["fusable"] and plan[e]["all"]["n_groups"] == 0
    assert plan["e_one_pose"]["stages"][0]["max_grp_fronts"] == 1 and not plan["e_one_pose"]["root"]["flow"] and plan["e_one_pose"]["stages"][0]["nw_flow"] == 0
    assert plan["e_small5"]["stages"][0]["max_grp_fronts"] == 3 and plan["e_small5"]["root"]["flow"] and plan["e_small5"]["root"]["nw"] == 3
    assert plan["f_a_no_preassemble"]["form"] == "band_stages" and not any(s["pre"] for s in plan["f_a_no_preassemble"]["stages"])
    nf = plan["f_a_no_solve_flow"]
    assert nf["form"] == "band_stages" and all(s["nw_flow"] == 0 for s in nf["stages"]) and not nf["root"]["flow"]
    assert any(s["nw_flow"] > 0 for s in plan["f_a_no_root_fuse"]["stages"])
    assert plan["f_a_no_root_fuse"]["form"] == "band_stages" and not plan["f_a_no_root_fuse"]["root"]["fusable"] and a["root"]["fusable"]
    pl = plan["f_a_plain_schedule"]
    assert pl["form"] == "band_stages" and not pl["root"]["fusable"] and not any(s["pre"] or s["nw_flow"] for s in pl["stages"])


def test_flow_waves_equal_the_two_expressions_they_replace(lib):
    """launch_band_solve sized the data flow against the 159 KB a launch may ask for, plan_chunks against the 150 KB planning budget"""
    budget, ceiling, cap, rows = lib.k3_const(0), lib.k3_const(1), lib.k3_const(3), lib.k3_const(5)
    assert (budget, ceiling, cap, rows) == (150 * 1024, 160 * 1024 - 1024, 12, 128)
    assert (lib.k3_const(2), lib.k3_const(4)) == (8, 8)
    rng = np.random.default_rng(7)
    for _ in range(200):
        max_panel, mg = int(rng.integers(1, 8001)), int(rng.integers(1, 41))
        per_wave = rows + max_panel                                   # doubles: xb + the factor panel
        assert lib.k3_solve_lds_bytes(max_panel) == 8 * per_wave
        fixed = (mg * rows + (mg + 1) // 2) * 8
        assert lib.k3_flow_fixed_bytes(mg) == fixed
        # launch_band_solve: room = limit > fixed ? (limit - fixed) / (per_wave * 8) : 0; nwf = min(min(12, mg), room)
        room = (ceiling - fixed) // (per_wave * 8) if ceiling > fixed else 0
        assert lib.k3_flow_waves(8 * per_wave, mg, cap, ceiling) == min(12, mg, room), (max_panel, mg)
        # plan_chunks: if (fixed + per_wave <= budget) nw_flow = max(1, min(min(12, mg), (budget - fixed) / per_wave)), else 0
        want = max(1, min(12, mg, (budget - fixed) // (8 * per_wave))) if fixed + 8 * per_wave <= budget else 0
        assert lib.k3_flow_waves(8 * per_wave, mg, cap, budget) == want, (max_panel, mg)


def fits_pre(counts, nw):
    """the shape test as run_analysis and plan_chunks each had it"""
    nl = len(counts)
    if not 1 <= nl <= 4:
        return False
    c0, upper = counts[0], sum(counts[1:])
    return c0 + upper <= nw or (nl >= 3 and c0 <= nw and upper <= nw)


def test_group_fits_pre(lib, dumps):
    def dev(counts, nw):
        glo, gfo = _i32([0, len(counts)]), _i32(np.concatenate([[0], np.cumsum(counts)]))
        return bool(lib.k3_group_fits_pre(glo.ctypes.data_as(_ip), gfo.ctypes.data_as(_ip), 0, nw))
    for counts, nw, want in (((8, 4, 2, 1), 8, True), ((4, 2, 1), 8, True), ((9, 4, 2, 1), 8, False), ((8, 4), 8, False), ((8, 4, 2, 1, 1), 8, False)):
        assert fits_pre(counts, nw) is want and dev(counts, nw) is want, (counts, nw)
    for name in ("a_corridor150", "b_corridor2000", "c_fronts_65_80"):
        A = dumps[name]
        glo, gfo = _i32(A["grp_lvl_off"]), _i32(A["glvl_front_off"])
        for gi in range(A["n_groups"]):
            counts = tuple(int(gfo[l + 1] - gfo[l]) for l in range(glo[gi], glo[gi + 1]))
            for nw in (1, 2, 4, 7, 8):
                assert bool(lib.k3_group_fits_pre(glo.ctypes.data_as(_ip), gfo.ctypes.data_as(_ip), gi, nw)) is fits_pre(counts, nw), (name, gi, counts, nw)
