"""Op-level tests of csrc/kernels/rouge.hip: ``counts`` EQUAL ``train.scst.rouge_ids`` for every row of
the launches of tests/rouge_cases.py, ``reward`` within 1e-6 relative of ``rouge_f`` of those counts in
float64 for all four ``--rl_reward`` choices (about 8 fp32 ulps for five operations of under 2 ulp each),
outputs inside sentinel allocations, rows independent of their place, the limit 256, and one pass of the
same launches through the bounds-checked library in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rouge_cases as C
from textsummarization_on_flink_amd.config import RL_REWARDS

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


@pytest.fixture(scope="module")
def cases():
    """The launches with the rule's counts, computed once."""
    Ls = C.launches()
    return [(L, C.want_counts(L)) for L in Ls]


def test_counts_and_rewards_equal_the_host_rule(cases):
    k = _ops()
    rows = sum(C.check(k, L, want) for L, want in cases)
    assert rows == 26 * C.R
    # what the launches reached: every length on both sides, both rows settings, the limit, every content
    hl = {len(h) for L, _ in cases for h in L["hyps"]}
    rl = {len(r) for L, _ in cases for r in L["refs"]}
    assert {0, 1, 2, 3, 63, 64, 65, 100, 128, 129, 256} <= hl | {x - 1 for x in hl}
    assert {0, 1, 2, 3, 63, 64, 65, 100, 128, 129, 256} <= rl | {x - 1 for x in rl}
    want = np.concatenate([w for _, w in cases])
    assert (want[:, 2] > 64).any() and (want[:, 3] == 0).any() and (want[:, 4] == 0).any()
    assert ((want[:, 0] > 0) & (want[:, 1] == 0)).any() and (want[:, 2] < want[:, 0]).any()


def test_stop_in_the_middle_and_no_stop(cases):
    """the planted [STOP] cuts the hypothesis; a hypothesis without one counts whole"""
    seen = 0
    for L, want in cases:
        if "stop_middle" in L["name"]:
            for r, h in enumerate(L["hyps"]):
                if len(h) >= 2:
                    assert want[r, 3] == h.index(C.STOP) <= len(h) // 2 < len(h)
                    seen += 1
        if "no_stop" in L["name"]:
            assert all(C.STOP not in h and want[r, 3] == len(h) for r, h in enumerate(L["hyps"]))
            seen += 1
    assert seen >= 10


@pytest.mark.parametrize("rows", [1, 2])
def test_permuting_the_rows_permutes_the_results(rows):
    k = _ops()
    L = C.launch("alphabet3", rows, seed=41)
    Na = C.R // rows
    pa = np.random.default_rng(rows).permutation(Na)
    pr = (pa[:, None] * rows + np.arange(rows)[None, :]).reshape(-1)  # the articles move with their rows
    P = dict(L, tok=L["tok"][:, pr], slen=L["slen"][pr], ref=L["ref"][pa], rlen=L["rlen"][pa])
    assert not np.array_equal(pr, np.arange(C.R))
    for kind in RL_REWARDS:
        c0, r0 = C.run(k, L, kind)
        c1, r1 = C.run(k, P, kind)
        assert np.array_equal(c1, c0[pr]) and np.array_equal(r1.view(np.int32), r0[pr].view(np.int32))
    # one row alone gives what it gives among six
    one = dict(L, tok=np.repeat(L["tok"][:, 4:5], C.R, 1), slen=np.repeat(L["slen"][4:5], C.R),
               ref=np.repeat(L["ref"][4 // rows:4 // rows + 1], Na, 0), rlen=np.repeat(L["rlen"][4 // rows:4 // rows + 1], Na))
    c2, r2 = C.run(k, one, "rouge_mean")
    c0, r0 = C.run(k, L, "rouge_mean")
    assert (c2 == c0[4]).all() and (r2.view(np.int32) == r0[4:5].view(np.int32)).all()


def test_binding_refuses_lengths_above_256_and_bad_arguments():
    k = _ops()
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    Rr = 4
    out = (z(Rr, 5), z(Rr, dt=torch.float32))
    k.rouge_reward(z(256, Rr), z(Rr), z(Rr, 256), z(Rr), *out, Rr, 256, 256, 1, C.STOP, 0)  # the limit itself
    with pytest.raises(RuntimeError, match="up to 256"):
        k.rouge_reward(z(257, Rr), z(Rr), z(Rr, 256), z(Rr), *out, Rr, 257, 256, 1, C.STOP, 0)
    with pytest.raises(RuntimeError, match="up to 256"):
        k.rouge_reward(z(256, Rr), z(Rr), z(Rr, 257), z(Rr), *out, Rr, 256, 257, 1, C.STOP, 0)
    with pytest.raises(RuntimeError, match="rouge_reward"):
        k.rouge_reward(z(8, Rr), z(Rr), z(Rr, 8), z(Rr), *out, Rr, 8, 8, 3, C.STOP, 0)  # rows does not divide R
    with pytest.raises(RuntimeError, match="rouge_reward"):
        k.rouge_reward(z(8, Rr), z(Rr), z(Rr, 8), z(Rr), *out, Rr, 8, 8, 1, C.STOP, 4)  # no such reward
    with pytest.raises(RuntimeError, match="ref"):
        k.rouge_reward(z(8, Rr), z(Rr), z(Rr, 8), z(Rr), *out, Rr, 8, 8, 2, C.STOP, 0)  # ref holds R rows, not R / 2
    with pytest.raises(RuntimeError, match="counts"):
        k.rouge_reward(z(8, Rr), z(Rr), z(Rr, 8), z(Rr), z(Rr, 4), out[1], Rr, 8, 8, 1, C.STOP, 0)


def test_lengths_past_the_buffers_are_clamped():
    """slen / ref_len beyond D / Lr (a corrupt book) read nothing outside the buffers: clamped to them"""
    k = _ops()
    L = C.launch("alphabet3", 1, seed=43)
    bad = dict(L, slen=L["slen"].copy(), rlen=L["rlen"].copy())
    bad["slen"][1], bad["rlen"][2], bad["slen"][3] = C.D + 50, C.D + 7, -4
    ok = dict(bad, slen=np.clip(bad["slen"], 0, C.D), rlen=np.clip(bad["rlen"], 0, C.D))
    c0, r0 = C.run(k, ok, "rouge_l")
    c1, r1 = C.run(k, bad, "rouge_l")
    assert np.array_equal(c0, c1) and np.array_equal(r0, r1)
    want = np.array([C.S.rouge_ids(ok["tok"][:ok["slen"][r], r], ok["ref"][r, :ok["rlen"][r]], C.STOP)
                     for r in range(C.R)])
    assert np.array_equal(c1, want)


CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import rouge_cases as C
from textsummarization_on_flink_amd import ops
k = ops.ops()
res = {"enabled": int(k.debug_enabled()), "lib": ops.library_path()}
k.debug_clear()
res["rows"] = sum(C.check(k, L) for L in C.launches()[::3])
torch.cuda.synchronize()
res["clean"] = [int(x) for x in k.debug_status().tolist()]
k.debug_clear()
L = C.launch("alphabet3", 1, seed=43)
L["slen"][1] = C.D + 50
C.run(k, L, "rouge_l")
torch.cuda.synchronize()
res["bad_slen"] = [int(x) for x in k.debug_status().tolist()]
k.debug_clear()
L = C.launch("alphabet3", 2, seed=44)
L["rlen"][2] = C.D + 7
C.run(k, L, "rouge_l")
torch.cuda.synchronize()
res["bad_rlen"] = [int(x) for x in k.debug_status().tolist()]
k.debug_clear()
print("RESULT " + json.dumps(res))
'''


def test_bounds_checked_library_runs_the_launches_clean():
    lib = os.path.join(REPO, "textsummarization_on_flink_amd", "_C_debug.so")
    assert os.path.exists(lib), "build the debug library first: python -m textsummarization_on_flink_amd._build"
    env = dict(os.environ, TSAMD_KERNEL_DEBUG="1", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(REPO, "tests")], env=env, capture_output=True,
                       text=True, timeout=240, cwd=REPO)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(line[0][7:])
    assert res["enabled"] == 1 and res["lib"].endswith("_C_debug.so")
    assert res["rows"] == 9 * C.R and res["clean"] == [0, 0, 0, 0], res
    assert res["bad_slen"][0] == 11 and res["bad_slen"][1] == 1 and res["bad_slen"][3] == C.D + 50, res
    assert res["bad_rlen"][0] == 12 and res["bad_rlen"][1] in (4, 5) and res["bad_rlen"][3] == C.D + 7, res
