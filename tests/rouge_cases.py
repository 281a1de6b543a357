"""Launches of ``rouge_reward`` (csrc/kernels/rouge.hip) and their check against the host rule of
train/scst.py, shared by tests/test_gpu_rouge_ops.py (release library) and its child process on the
bounds-checked library.

A launch is R = 6 hypothesis rows of ``rows`` (1 or 2) per article at D = Lr = 130 (one set at the limit
256).  Lengths come from LENS: an empty side, no bigram, the 64-token ballot-word boundary and the carry
into the second (third, fourth) word.  Contents: identical, disjoint, one token repeated, an alphabet
of 3, [STOP] in the middle of the hypothesis, a hypothesis without [STOP].  What lies past slen /
ref_len in the buffers are tokens that would match, so a kernel that read them would count too much."""
import numpy as np

from textsummarization_on_flink_amd.config import RL_REWARDS
from textsummarization_on_flink_amd.train import scst as S

STOP = 3
LENS = [0, 1, 2, 3, 63, 64, 65, 100, 128, 129]
CONTENTS = ("identical", "disjoint", "repeated", "alphabet3", "stop_middle", "no_stop")
R, D = 6, 130
SENT_I, SENT_F = -7777, 12288.0


def _fill(kind, rng, nh, nr):
    """(hypothesis tokens without [STOP], reference tokens without [STOP])"""
    if kind == "identical":
        x = rng.integers(4, 60, max(nh, nr))
        return x[:nh], x[:nr]
    if kind == "disjoint":
        return rng.integers(4, 500, nh), rng.integers(500, 1000, nr)
    if kind == "repeated":
        return np.full(nh, 9), np.full(nr, 9)
    if kind == "alphabet3":
        return rng.integers(4, 7, nh), rng.integers(4, 7, nr)
    return rng.integers(4, 12, nh), rng.integers(4, 12, nr)  # stop_middle / no_stop: a small alphabet


def launch(kind, rows, seed, d=D, lens=LENS):
    """One launch's buffers and the sequences the rule reads (the buffers up to slen / ref_len)."""
    rng = np.random.default_rng(seed)
    Na = R // rows
    tok = rng.integers(4, 12, (d, R)).astype(np.int32)
    ref = rng.integers(4, 12, (Na, d)).astype(np.int32)
    slen, rlen = np.zeros(R, np.int32), np.zeros(Na, np.int32)
    refs = []
    for a in range(Na):
        nr = int(lens[(seed + 3 * a) % len(lens)])
        refs.append(nr)
    hyps = []
    for r in range(R):
        a = r // rows
        nh, nr = int(lens[(seed * 7 + r) % len(lens)]), refs[a]
        h, rf = _fill(kind, np.random.default_rng(seed * 100 + a), max(nh, lens[-1]), nr)
        h = np.array(h[:nh])
        if rows > 1 and r % rows:  # the article's other rows: another hypothesis against the same reference
            h = np.roll(h, 1)
        if r % rows == 0:
            ref[a, :nr] = rf
            rlen[a] = nr
            if nr < d and a % 2 == 0:  # a target that ends in [STOP] (a truncated one does not)
                ref[a, nr] = STOP
                rlen[a] = nr + 1
        tok[:nh, r] = h
        slen[r] = nh
        if kind == "stop_middle" and nh >= 2:
            tok[nh // 2, r] = STOP  # the tokens after it do not count
        elif kind != "no_stop" and nh < d and r % 2 == 0:
            tok[nh, r] = STOP  # the sampler's own end: slen counts it
            slen[r] = nh + 1
        hyps.append(tok[:slen[r], r].tolist())
    return dict(name=f"{kind}/rows{rows}/seed{seed}/D{d}", tok=tok, slen=slen, ref=ref, rlen=rlen, rows=rows, d=d,
                hyps=hyps, refs=[ref[a, :rlen[a]].tolist() for a in range(Na)])


def launches():
    out = []
    for i, kind in enumerate(CONTENTS):
        for rows in (1, 2):
            out.append(launch(kind, rows, seed=2 * i + rows))
    for seed in range(20, 30):  # more length pairs over the tie-heavy alphabet
        out.append(launch("alphabet3", 1 + seed % 2, seed))
    big = [256, 255, 193, 192, 129, 64, 1, 0, 250, 200]
    for seed, kind in enumerate(("alphabet3", "identical", "repeated", "stop_middle")):
        out.append(launch(kind, 1 + seed % 2, seed, d=256, lens=big))
    return out


def f64(hit, n_hyp, n_ref):
    if hit == 0:
        return 0.0
    p, r = hit / n_hyp, hit / n_ref
    return 2.0 * p * r / (p + r)


def reward64(c, kind):
    hit1, hit2, lcs, nh, nr = (int(x) for x in c)
    f1, f2, fl = f64(hit1, nh, nr), f64(hit2, max(nh - 1, 0), max(nr - 1, 0)), f64(lcs, nh, nr)
    return {"rouge_l": fl, "rouge_1": f1, "rouge_2": f2, "rouge_mean": (f1 + f2 + fl) / 3.0}[kind]


def want_counts(L):
    return np.array([S.rouge_ids(h, L["refs"][r // L["rows"]], STOP) for r, h in enumerate(L["hyps"])], np.int32)


def run(k, L, kind, dev="cuda"):
    """(counts [R][5], reward [R]) of launch L from ops ``k``; the sentinels behind both outputs checked."""
    import torch
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    cfull = torch.full((R * 5 + 64,), SENT_I, dtype=torch.int32, device=dev)
    rfull = torch.full((R + 64,), SENT_F, dtype=torch.float32, device=dev)
    counts, reward = cfull[:R * 5].view(R, 5), rfull[:R]
    k.rouge_reward(t(L["tok"]), t(L["slen"]), t(L["ref"]), t(L["rlen"]), counts, reward, R, L["d"], L["d"], L["rows"],
                   STOP, RL_REWARDS.index(kind))
    assert bool((cfull[R * 5:] == SENT_I).all()) and bool((rfull[R:] == SENT_F).all()), L["name"]
    return counts.cpu().numpy(), reward.cpu().numpy()


def check(k, L, want=None):
    """Every reward choice of launch L: counts equal the rule, rewards within 1e-6 relative of float64.
    Returns the number of rows compared."""
    want = want_counts(L) if want is None else want
    for kind in RL_REWARDS:
        counts, reward = run(k, L, kind)
        assert np.array_equal(counts, want), (L["name"], kind, counts.tolist(), want.tolist())
        for r in range(R):
            w = reward64(want[r], kind)
            assert abs(float(reward[r]) - w) <= 1e-6 * w, (L["name"], kind, r, float(reward[r]), w)
            assert np.float32(reward[r]) == S.reward_from_counts(want[r], kind) or w > 0  # (0 exactly when no hit)
    return R
