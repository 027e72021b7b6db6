"""The GEMM's launch plan (csrc/gemm_plan.cpp, gemm_launch.h), checked on the host — no GPU needed.

wm_gemm_plan is the one place that decides which kernel family, tile, row-band schedule and grid a WmGemmArgs gets.  A stand-alone
program (tests/gemm_plan_table.cpp, its own main) is built from gemm_plan.cpp and wm_tuning.cpp alone and prints the plan of every case of
tests/gemm_plan_cases.h under every tuning setting (one line per case, tunings with the same plan sharing an entry); the table is compared with tests/golden/gemm_plan.json.  The rows at 256 CUs of that
file were proven equal to what the three former copies of the decision (plan_gemm, launch_T, launch_pp_E of the single gemm.hip) launched;
the rows at 64 CUs were added from this program afterwards.
"""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "hunyuanworld-mirror_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    d = tmp_path_factory.mktemp("gemm_plan")
    objs = []
    for src in (os.path.join(CSRC, "gemm_plan.cpp"), os.path.join(CSRC, "wm_tuning.cpp"), os.path.join(TESTS, "gemm_plan_table.cpp")):
        obj = str(d / (os.path.basename(src) + ".o"))
        r = subprocess.run(["hipcc", "-O1", "-std=c++17", "-x", "hip", "--cuda-host-only", "-I", CSRC, "-I", TESTS, "-c", src, "-o", obj],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        objs.append(obj)
    exe = str(d / "gemm_plan_table")
    r = subprocess.run(["hipcc", *objs, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return {"objs": objs, "doc": json.loads(r.stdout), "rows": _rows(json.loads(r.stdout))}


def _rows(doc):
    """One dict per (case, tuning, ncu): a line of the document holds a case with its plans, each plan with the tunings that give it."""
    out = []
    for line in doc["rows"]:
        case = dict(zip(doc["columns"]["case"], line))
        for plan in case.pop("plans"):
            p = dict(zip(doc["columns"]["plan"], plan))
            for tuning in p.pop("tunings"):
                out.append({**case, **p, "tuning": doc["tunings"][tuning]})
    return out


def test_plan_program_calls_no_hip_runtime_function(table):
    for obj in table["objs"]:
        r = subprocess.run(["nm", "-u", obj], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        undefined = [l.split()[-1] for l in r.stdout.splitlines() if l.strip()]
        assert not [s for s in undefined if s.lower().startswith(("hip", "__hip", "hsa"))], (obj, undefined)


def test_plan_table_matches_the_committed_one(table):
    want = json.load(open(os.path.join(TESTS, "golden", "gemm_plan.json")))
    got = table["doc"]
    assert got["columns"] == want["columns"] and got["tunings"] == want["tunings"]
    g_rows, w_rows = table["rows"], _rows(want)
    assert len(g_rows) == len(w_rows) and len(g_rows) > 2000
    for g, w in zip(g_rows, w_rows):
        assert g == w, (g, w)
    assert got["rows"] == want["rows"]


def test_plan_invariants(table):
    """What the three copies of the decision used to leave implicit, for every row."""
    tiles = {0: (128, 128), 1: (256, 128), 2: (256, 128), 3: (256, 256), 4: (256, 256), 5: (192, 256), 6: (256, 256)}   # gemm_nt.hip's table
    EPI_RESID, EPI_CONV = 3, 7
    n = {"NT32": 0, "NT16": 0, "PP1": 0, "PP2": 0, "-": 0, "bands": 0, "fuses": 0, "pf": 0}
    for r in table["rows"]:
        n[r["family"]] += 1
        if r["err"]:
            assert r["family"] == "-"
            continue
        assert r["family"] in ("NT32", "NT16", "PP1", "PP2") and 0 <= r["cfg"] <= 6, r
        if r["family"] != "NT32":
            assert r["cfg"] in (4, 5), r
        if r["family"] in ("PP1", "PP2"):
            assert r["qi"] == (3 if r["cfg"] == 5 else 4), r
        assert (r["ver"] in (2, 3)) == (r["family"] == "PP2"), r
        if r["bands"] > 0:
            n["bands"] += 1
            assert r["family"] == "PP2", r
            units, full = (r["M"] + 15) // 16, 16 if r["cfg"] == 4 else 12
            assert -(-units // r["bands"]) <= full and units // r["bands"] >= full - 4, r   # what gemm_pp2_kernel's instantiations cover
        if r["fuses_ln"]:
            n["fuses"] += 1
            rows = r["bands"] if r["bands"] > 0 else -(-r["M"] // 192)
            assert r["family"] == "PP2" and r["cfg"] == 5 and r["epi"] == EPI_RESID and r["N"] == 1024 and rows * 4 <= r["ncu"], r
        if r["pf_c"]:
            n["pf"] += 1
            assert r["epi"] == EPI_RESID, r
        if r["epi"] == EPI_CONV:
            assert r["family"] == "PP2" and r["ver"] == 2, r
        bm, bn = tiles[r["cfg"]]
        rows = r["bands"] if r["bands"] > 0 else -(-r["M"] // bm)
        assert r["grid"] == rows * -(-r["N"] // bn), r
        assert r["block"] == (256 if r["cfg"] == 0 else 512), r
        assert 0 < r["lds"] <= 160 * 1024, r
    # the table reaches every family, the schedule, the fused epilogue, the prefetch and a refused launch
    assert all(v > 0 for v in n.values()), n
