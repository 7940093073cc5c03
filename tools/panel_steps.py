#!/usr/bin/env python
"""Instructions per panel step of the register-tile elimination, from the gfx950 assembly (no GPU needed): DESIGN.md section 8 1g.

  python tools/panel_steps.py [--filter REGEX] [--asm FILE.s] [--check]

Compiles pop_up_slam_amd/csrc/pps_k3.hip device-only with the Makefile's flags and -S (or reads FILE.s), and in every kernel looks for
the 4 x 4 pivot blocks of pps_front_reg.h: four v_rsq_f64 close together (chol4).  A panel step is
  - the body of the innermost loop around a pivot block, when that loop holds no other pivot block (the loop proper), or
  - the instructions from this pivot block to the next one, for steps in straight-line code (peeled by the compiler, or the unrolled
    tile columns of kFlat4); the last of them in front of a loop ("handover") also holds that loop's prologue.
Per step: instructions, VALU (v_* without MFMA), SALU (s_*), LDS (ds_*), MFMA, v_mov_b64 (a tile copy is two of them) and s_nop.
--check: exit status 1 unless every step of every kernel shown stays within 10 % of the kernel's first step of the same tile count
(MFMAs of a column-0 step: 10, 6, 3 tiles) and holds at most 2 v_mov_b64 -- the condition the 4-column kernels are held to.
The verdict is ADVISORY: the tool measures spans of text, not executed paths.  The fourth step of an unrolled column ("handover") is shown
with whatever is laid out behind it and is exempt; in k_band_factor_lean_trace an out-of-line block of the clock reads is taken for a loop
of 419 instructions and reported, so --check exits 1 on the default filter although the step is the 231 of its neighbours.  Where a span
looks too long, read the executed path in the assembly (DESIGN.md section 8 1g does so for the hand-over step of k_band_factor<true>).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pop_up_slam_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast-honor-pragmas", "--cuda-device-only", "-S"]
GROUP_SPAN = 120        # the four reciprocal square roots of one chol4 lie within this many instructions (measured: about 80)


def kernels(text):
    """{mangled name: [(mnemonic, operand text) | ('label', name)]} of every function of the assembly"""
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            cur.append(("label", m.group(1)))
            continue
        s = line.strip()
        if not s or s[0] in ".;" or not line[:1].isspace():
            continue
        f = s.split(None, 1)
        cur.append((f[0], f[1] if len(f) > 1 else ""))
    return out


def steps(items):
    ins = [(i, it) for i, it in enumerate(items) if it[0] != "label"]         # position in `items` of every instruction
    label_at = {it[1]: i for i, it in enumerate(items) if it[0] == "label"}
    rsq = [i for i, it in ins if it[0].startswith("v_rsq_f64")]
    groups = []
    for i in rsq:
        if groups and len(groups[-1]) < 4 and i - groups[-1][0] < 2 * GROUP_SPAN:
            groups[-1].append(i)
        else:
            groups.append([i])
    groups = [g[0] for g in groups if len(g) == 4]
    loops = []                                                                # (first item, last item) of every backward branch
    for i, it in ins:
        if it[0].startswith(("s_cbranch", "s_branch")) and it[1].split()[0] in label_at and label_at[it[1].split()[0]] <= i:
            loops.append((label_at[it[1].split()[0]], i))
    out = []
    for k, g in enumerate(groups):
        # (a step ends with its trailing update: a backward jump of a block laid out of line, as the trace kernels have them, is no step's loop)
        own = [(a, b) for a, b in loops if a <= g <= b and sum(a <= h <= b for h in groups) == 1 and any(it[0].startswith("v_mfma") for it in items[a:b + 1])]
        if own:
            a, b = min(own, key=lambda ab: ab[1] - ab[0])
            kind = "loop"
        elif k + 1 < len(groups):
            a, b, kind = g, groups[k + 1] - 1, "straight"
            # the last straight-line step of an unrolled column runs on into what is laid out behind it -- the exits of the steps before it, the
            # prologue of the next column's loop (its rotated trailing update included) or the tile load of the next elimination: counted,
            # shown as "handover", not held to the condition of --check (DESIGN.md gives the executed path of such a step)
            if any(la <= groups[k + 1] <= lb and sum(la <= h <= lb for h in groups) == 1 for la, lb in loops):
                kind = "handover"
        else:
            continue                                                          # (the last block of a kernel outside any loop: no end to count to)
        if kind == "straight" and len(out) >= 3 and all(out[-j]["kind"] == "straight" and out[-j]["start"] == groups[k - j] for j in (1, 2, 3)):
            kind = "handover"                                                 # the fourth step of an unrolled column: what follows it in the text is not a step
        body = [it for it in items[a:b + 1] if it[0] != "label"]
        n = lambda pred: sum(1 for it in body if pred(it[0]))
        out.append({"kind": kind, "start": g, "instr": len(body), "valu": n(lambda m: m.startswith("v_") and not m.startswith("v_mfma")),
                    "salu": n(lambda m: m.startswith("s_")), "lds": n(lambda m: m.startswith("ds_")), "mfma": n(lambda m: m.startswith("v_mfma")),
                    "mov64": n(lambda m: m.startswith("v_mov_b64")), "nop": n(lambda m: m == "s_nop")})
    return out


def demangle(n):
    try:
        return re.sub(r"\(.*", "", subprocess.check_output(["c++filt", n], text=True).strip()).replace("pps::", "").replace("void ", "")
    except Exception:
        return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", default="k_band_factor_all|k_band_factor_pre|kb_band_factor_pre|k_band_root<true|band_factor<true>|lean_trace")
    ap.add_argument("--asm", default="")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, "k3.s")
            subprocess.check_call(["/opt/rocm/bin/hipcc"] + FLAGS + [os.path.join(CSRC, "pps_k3.hip"), "-o", out], stderr=subprocess.DEVNULL)
            text = open(out).read()
    bad = 0
    print(f"{'kernel':<34} {'step':>4} {'form':<8} {'instr':>5} {'VALU':>5} {'SALU':>5} {'LDS':>4} {'MFMA':>4} {'mov64':>5} {'s_nop':>5}")
    for name, items in sorted(kernels(text).items(), key=lambda kv: demangle(kv[0])):
        short = demangle(name)
        if not re.search(a.filter, short):
            continue
        st = steps(items)
        first, prev = None, None
        for k, s in enumerate(st):
            # a column-0 step (10, 6 or 3 tiles) with more tiles than the step before it: the elimination of the next tile count starts, and its
            # steps are held against this one.  (A hand-over span counts MFMAs of two steps and is neither a reference nor a predecessor.)
            if s["kind"] != "handover":
                if s["mfma"] in (10, 6, 3) and (prev is None or s["mfma"] > prev["mfma"]):
                    first = s
                prev = s
            over = first is not None and s["kind"] != "handover" and (s["instr"] > 1.10 * first["instr"] or s["mov64"] > 2)
            bad += over
            print(f"{short:<34} {k:>4} {s['kind']:<8} {s['instr']:>5} {s['valu']:>5} {s['salu']:>5} {s['lds']:>4} {s['mfma']:>4} {s['mov64']:>5} {s['nop']:>5}"
                  + ("   <-- over" if over else ""))
    if a.check and bad:
        print(f"{bad} step(s) beyond 110 % of their kernel's first step or with more than 2 v_mov_b64")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
