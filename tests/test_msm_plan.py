"""csrc/msm_plan.h on its own: tests/cpp/msm_plan_main.cpp -- a stand-alone program that includes nothing but that header -- built with
host clang++ -fsanitize=address,undefined -fno-sanitize-recover and run directly.  It sweeps the shape of a large-MSM call (both groups,
n up to 2^27 and +-1 where the endomorphism split switches off, every forced window 4..16, every table window 9..21, images, no_glv,
force_slow_sort, an item cap of 16), checks every accepted shape, its buffer sizes and its reduction schedule, reaches each of the three
refusals with one call, and prints every shape and schedule.  The printed lines are compared here with tests/msm_pipe_model.py, whose
`pick_window` and `reduction_schedule` were written from the description of the plan, not from the header: the independent check that
the header says what msm_device did before it launched from it.  Nothing here is loaded into Python."""
import os
import re
import subprocess

import pytest

import msm_pipe_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(ROOT, "tests", "cpp", "msm_plan_main.cpp")
CSRC = os.path.join(ROOT, "bls12_381_amd", "csrc")
HDRS = [os.path.join(CSRC, "msm_plan.h"), os.path.join(CSRC, "limits.h")]
EXE = os.path.join(ROOT, "build", "msm_plan_main")


@pytest.fixture(scope="module")
def output():
    """the program under the address and undefined-behaviour sanitizers: every check passes and nothing is reported"""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [SRC] + HDRS):
        tmp = EXE + ".tmp%d" % os.getpid()
        subprocess.check_call([CLANG, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-iquote", CSRC, SRC, "-o", tmp])
        os.replace(tmp, EXE)
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, "exit status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return p.stdout.splitlines()


def test_plan_program_runs_clean(output):
    for part in ("sweep", "refusals"):
        assert part in output, "the program did not reach '%s'" % part
    assert output[-1] == "all ok"


def test_shapes_match_the_model(output):
    """every shape line against the model: the decomposition rule, `pick_window`, `nwin_of`, `sort_split`, `item_cap` and the three
    refusals by their conditions"""
    lines = [l for l in output if l.startswith("shape ")]
    assert len(lines) == 2 * 34 * 27 * 16
    seen = set()
    for line in lines:
        f = {k: v for k, v in re.findall(r"(\w+)=(\S+)", line)}
        refusal = f.pop("refusal")
        f = {k: int(v) for k, v in f.items()}
        group, n, merged = f["group"], f["n"], f["table_c"] != 0
        split = not merged and f["images"] and not f["no_glv"] and not f["slow"]
        words = 4 if group == 1 and split and 2 * n <= 1 << 24 else 2 if group == 2 and split and 4 * n <= 1 << 24 else 8
        ns, sbits = n * (8 // words), mm.SBITS[words]
        c = f["table_c"] or f["msm_c"] or mm.pick_window(ns, sbits)
        nwin = mm.nwin_of(c, words)
        nseg, nbw = (1 if merged else nwin), 1 << (c - 1)
        fine, ncoarse, nc = mm.sort_split(c, nwin, merged)
        cap = mm.item_cap(ns, c, f["item_cap"])
        fast = merged or (ns <= 1 << 24 and c <= 16 and not f["slow"])
        total, nb = nwin * ns, nseg * nbw
        items = total // cap + nb + 1
        want = {"glv": int(words == 4), "gls": int(words == 2), "ns": ns, "sbits": sbits, "cw": c, "nwin": nwin, "nseg": nseg, "nbw": nbw, "nb": nb, "total": total,
                "fast": int(fast), "fine": fine, "ncoarse": ncoarse, "nc": nc, "cap": cap, "items": items, "records": nb + items}
        assert {k: f[k] for k in want} == want, line
        why = "entries" if total > 0xfffffff0 else "counters" if fast and nc > mm.SORT_MAX_COUNTERS else "fallback" if not fast and -(-nb // 1024) > 4096 else "none"
        assert refusal == why, line
        if why == "none":
            seen.add((nseg, nbw))
    scheds = [l for l in output if l.startswith("sched ")]
    assert sorted((int(a), int(b)) for a, b in (re.match(r"sched nseg=(\d+) nbw=(\d+) ", l).groups() for l in scheds)) == sorted(seen)


def test_schedules_match_the_model(output):
    """every schedule line -- levels, forms, grids, T offsets, the tree passes of every step, the Horner shifts -- is the model's"""
    scheds = [l for l in output if l.startswith("sched ")]
    assert len(scheds) == 3 * 13 + 13                                # windows 4..16 at 256, 128 and 64 bits; tables 9..21
    forms = set()
    for line in scheds:
        nseg, nbw = map(int, re.match(r"sched nseg=(\d+) nbw=(\d+) ", line).groups())
        assert line == mm.schedule_text(nseg, nbw)
        s = mm.reduction_schedule(nseg, nbw)
        forms |= {lv["form"] for lv in s["levels"]}
        # every tree finishes within the steps of the levels: nothing is left when the last level has run
        assert len(s["levels"]) <= 7 and len(s["steps"]) == len(s["levels"])
    assert forms == {0, 1, 2}


def test_schedule_computes_the_window_sum():
    """walking the model's schedule over integers -- levels, tree passes into the Horner rows, shifts -- gives sum_b (b + 1) e_b"""
    from oracle import bls12_381_ref as o
    r = o.SplitMix64(0x5c4ed)
    for nbw in (8, 16, 128, 1024, 1 << 15):
        E = [r.next() % 1000 for _ in range(nbw)]
        s = mm.reduction_schedule(1, nbw)
        rows, cur, tbuf = {}, E, {}
        for l, (lv, (_, _, passes)) in enumerate(zip(s["levels"], s["steps"])):
            cur, T = mm.level_sums(cur, lv["M"], lv["off"])
            if lv["horner"]:
                rows[l] = T[0]
            else:
                tbuf[(l, -1)] = T
            for (tl, n, tm, tg, src, pp, horner, _, _) in passes:
                t = tbuf[(tl, src)]
                assert len(t) == n
                out = [sum(t[g * tm:(g + 1) * tm]) for g in range(tg)]
                if horner:
                    rows[tl] = out[0]
                else:
                    tbuf[(tl, pp)] = out
        acc = rows[len(s["levels"]) - 1]
        for l, k in zip(range(len(s["levels"]) - 2, -1, -1), s["horner"]):
            acc = rows[l] + (acc << k)
        assert acc == sum((b + 1) * e for b, e in enumerate(E)), nbw


def test_the_restated_limits_match_their_origin():
    """the constants msm_plan.h restates from device headers (api_msm.hip static_asserts them at build time) and the model's copies"""
    plan = open(HDRS[0]).read()
    msm = open(os.path.join(CSRC, "msm.hip.h")).read()
    team = open(os.path.join(CSRC, "team.hip.h")).read()
    val = lambda text, pat: int(re.search(pat, text).group(1))
    assert val(plan, r"MSMP_TEAM = (\d+);") == val(team, r"constexpr int TEAM = (\d+);") == mm.TEAM
    assert val(plan, r"MSMP_SORT_MAX_COUNTERS = (\d+);") == val(msm, r"constexpr int SORT_MAX_COUNTERS = (\d+);") == mm.SORT_MAX_COUNTERS
    assert val(plan, r"MSMP_TREE_JOBS_MAX = (\d+);") == val(msm, r"constexpr int TREE_JOBS_MAX = (\d+);") == mm.TREE_JOBS_MAX
    assert val(plan, r"TEAM_LANES_MAX = (\d+);") == mm.TEAM_LANES_MAX and val(plan, r"MSMP_BLOCK = (\d+);") == mm.REDUCTION_BLOCK
