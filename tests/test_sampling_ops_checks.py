"""CPU tier of tests/test_gpu_sampling_ops.py: the exact inputs of tests/sampling_exact.py meet their own
conditions (asserted on the float64 reference alone), a numpy fp32 emulation of the PARALLEL form of
``sample_full`` (256-entry chunks, ``per`` chunks per thread, the 4-per-lane segment scan, min / max over
the crossing and last-positive chunks, ``sf_walk``) and of ``sample_topk`` equals ``draw_full`` /
``draw_topk`` on every exact row, and each planted mistake in that emulation is rejected by a named
launch (profiles/sampling_op_tests.md holds the table)."""
import numpy as np
import pytest

import sampling_exact as X
from sampling_exact import MIN_DEC, SEED, STOP, U
from textsummarization_on_flink_amd.decode.sampling import draw_full, sample_uniform

f32 = np.float32
NINF = f32(-np.inf)

# name: (the launch that must reject it, what it is)
MUTATIONS = {
    "ge_chunk": ("v3000_t2", ">= for > at the chunk crossing"),
    "ge_walk": ("v256_t2", ">= for > in the walk"),
    "no_w": ("clamp_u1", "no w > 0 test"),
    "own_up": ("v70000_t2", "own = cstar / per rounded up"),
    "seg_shift": ("v70000n_t2", "segment base shifted by one thread"),
    "mask_sum_only": ("v3000s_t2", "[STOP] masked in the chunk sum but not in the walk"),
    "mask_walk_only": ("v256_t2", "[STOP] masked in the walk but not in the chunk sum"),
    "ncp_T": (None, "ncp from T (the added chunks weigh 0: no exact input can tell)"),
    "len_T": ("v257_t3", "positions not cut at the article's length"),
    "entry_plus1": ("v64_t2", "position entry V + i + 1"),
    "art_mod": ("v257_t3", "art = r % rows"),
    "read_past": ("v3001_t3", "straddling lane reads past V"),
    "rank_le": ("K4_k3_t3_temp1.0_L-1.5", "top-k rank <= k"),
    "lt_k_first": ("K9_k8_t2_temp1.0_L-1.5", "top-k taking lane < k before dropping [STOP]"),
    "tail_done": ("book", "the tail writing done rows"),
}
FULL_MUTS = [m for m in MUTATIONS if m not in ("rank_le", "lt_k_first", "tail_done")]


def fexp(x):
    with np.errstate(all="ignore"):
        return np.exp2((np.asarray(x, f32) * f32(1.4426950408889634)).astype(f32)).astype(f32)


def emu_walk(w, rem, mut=None):
    """sf_walk: w [256] fp32, lane l owns entries 4 l .. 4 l + 3."""
    w4 = w.reshape(64, 4)
    inn = np.cumsum(w4, axis=1, dtype=f32)
    c = np.cumsum(inn[:, 3], dtype=f32)
    base = np.concatenate([[f32(0)], c[:-1]]).astype(f32)
    cum = (base[:, None] + inn).astype(f32)
    pos = np.ones_like(w4, bool) if mut == "no_w" else w4 > 0
    hit = pos & ((cum >= rem) if mut == "ge_walk" else (cum > rem))
    if hit.any():
        return int(np.nonzero(hit.ravel())[0][0])
    if pos.any():
        return int(np.nonzero(pos.ravel())[0][-1])
    return -1


def emu_full(L, r, mut=None, u=None):
    """sample_full_kernel for row r of launch L: (entry, token)."""
    V, T, rows, stop, t, R = L["V"], L["T"], L["rows"], L["stop"], L["t"], L["R"]
    art = (r % rows) % (R // rows) if mut == "art_mod" else r // rows
    ptr = L["ptr"]
    pg = f32(L["pg"][r]) if ptr else f32(1)
    ln = min(max(int(L["lens"][art]), 0), T) if ptr else 0
    allow = t >= MIN_DEC
    ncv = (V + 255) // 256
    ncp = ((T if mut == "ncp_T" and ptr else ln) + 255) // 256
    nch = ncv + ncp
    ex, a = L["ext"][art], L["attn"][r]
    x = np.full(ncv * 256, NINF, f32)
    x[:V] = L["logits"][r] + L["bias"]
    if mut == "read_past" and V % 4:
        flat = L["logits"].ravel()
        for v in range(V, (V + 3) // 4 * 4):
            x[v] = flat[r * V + v] if r * V + v < len(flat) else f32(0)
    ids = np.arange(ncv * 256)
    xc = x.reshape(ncv, 256)
    m = xc.max(1)
    with np.errstate(all="ignore"):
        e = np.where(m[:, None] > NINF, fexp(xc - m[:, None]), f32(0)).astype(f32)
    s = e.sum(1, dtype=f32)
    stop_chunk = stop // 256 if (not allow and 0 <= stop < V) else -1
    M = m.max()
    with np.errstate(all="ignore"):
        fm = fexp(m - M)
        S = f32((s * fm).sum(dtype=f32))
        scale = f32(pg / S)
        cw = np.zeros(nch, f32)
        sv = s.copy()
        if stop_chunk >= 0 and mut != "mask_walk_only":
            e2 = e[stop_chunk].copy()
            e2[stop - stop_chunk * 256] = 0
            sv[stop_chunk] = e2.sum(dtype=f32)
        cw[:ncv] = (scale * sv * fm).astype(f32)
        wv = np.where((ids < V), (scale * fexp(x - M)).astype(f32), f32(0)).astype(f32)
    if not allow and mut != "mask_sum_only":
        wv[ids == stop] = 0
    if ncp:
        i = np.arange(ncp * 256)
        cut = T if mut == "len_T" else ln
        inb = i < cut
        ii = np.minimum(i, T - 1)
        wp = np.where(inb, (f32(1) - pg) * a[ii], f32(0)).astype(f32)
        is_stop = inb & (ex[ii] == stop)
        wp_sum, wp_walk = wp.copy(), wp.copy()
        if not allow:
            if mut != "mask_walk_only":
                wp_sum[is_stop] = 0
            if mut != "mask_sum_only":
                wp_walk[is_stop] = 0
        cw[ncv:] = wp_sum.reshape(ncp, 256).sum(1, dtype=f32)
    # scan: thread q owns chunks q * per .. (q + 1) * per - 1
    per = (nch + 255) // 256
    pad = np.zeros(256 * per, f32)
    pad[:nch] = cw
    arr = pad.reshape(256, per)
    seg = arr.sum(1, dtype=f32) if per == 1 else np.cumsum(arr, axis=1, dtype=f32)[:, -1]
    v4 = seg.reshape(64, 4)
    inn = np.cumsum(v4, axis=1, dtype=f32)
    c = np.cumsum(inn[:, 3], dtype=f32)
    base = np.concatenate([[f32(0)], c[:-1]]).astype(f32)
    segx = np.concatenate([base[:, None], (base[:, None] + inn[:, :3]).astype(f32)], axis=1).ravel()
    W = c[-1]
    uu = f32(sample_uniform(SEED, L["streams"][r], t) if u is None else u)
    target = f32(uu * W)
    start = np.concatenate([segx[1:], segx[-1:]]) if mut == "seg_shift" else segx
    runs = (start[:, None] + np.cumsum(arr, axis=1, dtype=f32)).astype(f32)
    valid = (np.arange(256 * per) < nch).reshape(256, per)
    pos = valid & (np.ones_like(valid) if mut == "no_w" else arr > 0)
    hit = pos & ((runs >= target) if mut == "ge_chunk" else (runs > target))
    clamped = not hit.any()
    if clamped:
        if not pos.any():
            return -1, stop
        cstar = int(np.nonzero(pos.ravel())[0][-1])
    else:
        cstar = int(np.nonzero(hit.ravel())[0][0])
    own = min(-(-cstar // per) if mut == "own_up" else cstar // per, 255)
    before = segx[own]
    for cc in range(own * per, cstar):
        before = f32(before + cw[cc])
    rem = f32(np.inf) if clamped else f32(target - before)
    if cstar < ncv:
        e_ = emu_walk(wv[cstar * 256:(cstar + 1) * 256], rem, mut)
        return (cstar * 256 + e_, cstar * 256 + e_) if e_ >= 0 else (-1, stop)
    p = cstar - ncv
    e_ = emu_walk(wp_walk[p * 256:(p + 1) * 256], rem, mut)
    if e_ < 0:
        return -1, stop
    i = min(p * 256 + e_, T - 1)
    return V + i + (mut == "entry_plus1"), int(ex[i])


def emu_topk(L, r, mut=None):
    K, k, t = L["K"], L["k"], L["t"]
    lane = np.arange(64)
    ids, lp = np.full(64, -1), np.full(64, NINF, f32)
    ids[:K], lp[:K] = L["ids"][r], L["lp"][r]
    allow = t >= MIN_DEC
    if mut == "lt_k_first":
        keep = (lane < k) & (lane < K) & (allow | (ids != STOP))
    else:
        valid = (lane <= k) & (lane < K) & (allow | (ids != STOP))
        rank = np.cumsum(valid) - valid
        keep = valid & ((rank <= k) if mut == "rank_le" else (rank < k))
    if not keep.any():
        return 0
    m = lp[keep].max()
    with np.errstate(all="ignore"):
        w = np.where(keep, np.exp(((lp - m) / f32(L["temp"])).astype(f32)).astype(f32), f32(0)).astype(f32)
    c = np.cumsum(w, dtype=f32)
    target = f32(f32(sample_uniform(SEED, L["streams"][r], t)) * c[63])
    cross = keep & (w > 0) & (c > target)
    pos = keep & (w > 0)
    return int(lane[cross][0] if cross.any() else (lane[pos][-1] if pos.any() else lane[keep][0]))


def old_window_passes(L, r, pick, tok):
    """test_gpu_sampling._check_full_row's draw checks with its eps formula (logit range over the finite
    entries; -inf entries put the formula past its cap)."""
    w = X.full_weights(L, r)
    if not (0 <= pick < len(w)) or w[pick] <= 0:
        return False
    eps = 0.999e-3
    c = np.cumsum(w)
    x = sample_uniform(SEED, L["streams"][r], L["t"]) * c[-1]
    return bool(c[pick] - w[pick] - eps * c[-1] <= x <= c[pick] + eps * c[-1])


# ------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def full():
    return X.full_launches()


def test_exact_full_inputs_meet_their_conditions(full):
    rows = ties = 0
    for L in full:
        ties += sum(X.check_full(L))
        rows += L["R"]
        for E in X.extra_draws(L):
            X.check_full(E)
            rows += E["R"]
    print(f"sample_full: {rows} exact rows in {len(full)} launches, {ties} with a prefix sum equal to u * W")
    assert rows == X.FULL_ROWS and ties >= 50
    assert {L["V"] for L in full} == {64, 256, 257, 3000, 3001, 70000, 140000, 524288}
    assert {1, 255, 256, 257, 512, 2048} <= {L["T"] for L in full} | {int(n) for L in full for n in L["lens"]}
    assert {L["rows"] for L in full} == {1, 3} and any(max(L["streams"]) > 2 ** 32 for L in full)
    per = {((L["V"] + 255) // 256 + (int(L["lens"].max()) + 255) // 256 + 255) // 256 for L in full if L["ptr"]}
    assert per == {1, 2, 3, 9}


def test_emulation_equals_host_rule_on_every_exact_full_row(full):
    for L0 in full:
        for L in [L0] + X.extra_draws(L0):
            for r in range(L["R"]):
                assert emu_full(L, r) == (L["want_pick"][r], L["want_tok"][r]), (L["name"], r, L["streams"][r])


def test_exact_topk_inputs_and_emulation():
    rows = 0
    for L in X.topk_launches():
        want = X.check_topk(L)
        got = [emu_topk(L, r) for r in range(L["R"])]
        assert got == want.tolist(), L["name"]
        rows += L["R"]
    assert rows == X.TOPK_ROWS


def _clamp_case(full, mut):
    """u = 1.0 (no device uniform reaches it): no crossing, the last entry of positive weight.  The rows end in
    zero-weight entries (positions past the length, -inf logits), which the w > 0 tests must skip."""
    bad = []
    for L in full:
        if L["V"] > 3001:
            continue
        for r in range(L["R"]):
            vd, a64, pg, e, n = X.full_reference(L, r)
            want = draw_full(vd, a64, pg, e, n, 1.0, L["stop"], L["t"] >= MIN_DEC)
            if emu_full(L, r, mut, u=1.0) != want:
                bad.append((L["name"], r))
    return bad


def test_clamp_to_the_last_positive_entry(full):
    assert _clamp_case(full, None) == []


@pytest.mark.parametrize("mut", FULL_MUTS)
def test_planted_mistake_in_sample_full_is_rejected(full, mut):
    named = MUTATIONS[mut][0]
    if named == "clamp_u1":
        assert _clamp_case(full, mut)
        assert all(emu_full(L, r, mut) == (L["want_pick"][r], L["want_tok"][r])
                   for L in full if L["V"] <= 3001 for r in range(L["R"]))  # at a device uniform nothing tells
        return
    bad, passes_old = {}, 0
    for L in full:
        if L["V"] > 70000 and L["name"] != named:
            continue
        for r in range(L["R"]):
            got = emu_full(L, r, mut)
            if got != (L["want_pick"][r], L["want_tok"][r]):
                bad.setdefault(L["name"], []).append(r)
                if L["name"] == named:
                    passes_old += old_window_passes(L, r, *got)
    print(f"{mut}: rejected by {sorted(bad)}; in {named}: rows {bad.get(named)}, {passes_old} inside the old window")
    if named is None:
        assert not bad  # equivalent on exact inputs: the extra chunks weigh 0 and every sum is exact
    else:
        assert named in bad


@pytest.mark.parametrize("mut", ["rank_le", "lt_k_first"])
def test_planted_mistake_in_sample_topk_is_rejected(mut):
    bad = [L["name"] for L in X.topk_launches()
           if [emu_topk(L, r, mut) for r in range(L["R"])] != X.check_topk(L).tolist()]
    print(f"{mut}: rejected by {len(bad)} launches")
    assert MUTATIONS[mut][0] in bad


def _emu_tail(st, t, tok, lp, att, pg, stop, max_dec, mut=None):
    """the kernels' early return and sample_book, row by row"""
    for r in range(len(st["done"])):
        if t < 0 or t >= max_dec or (st["done"][r] and mut != "tail_done"):
            continue
        if "att_hist" in st:
            for lane in range(64):
                for i in range(lane, att.shape[1], 64):
                    st["att_hist"][t, r, i] = att[r, i]
        st["tok_hist"][t, r], st["lp_hist"][t, r] = tok[r], lp[r]
        st["lp_sum"][r] += f32(lp[r])
        st["latest"][r], st["slen"][r] = tok[r], t + 1
        if tok[r] == stop:
            st["done"][r] = 1
        if "pg_hist" in st:
            st["pg_hist"][t, r] = pg[r]


def book_drive(T, att, pg, mut=None):
    rng = np.random.default_rng(T)
    R, max_dec = 6, 4
    a, b = X.book_state(R, T, max_dec, att, pg), X.book_state(R, T, max_dec, att, pg)
    for t in (-1, 0, 1, 2, 3, 4):
        tok = rng.integers(10, 50, R)
        tok[[r for r in range(R - 1) if r % 3 == t - 1]] = STOP  # rows 0, 3 end at t = 1; 1, 4 at 2; 2 at 3; 5 never
        lp = -rng.random(R).astype(f32)
        A, P = rng.random((R, T)).astype(f32), rng.random(R).astype(f32)
        X.book_step(a, t, tok, lp, A, P, STOP, max_dec)
        _emu_tail(b, t, tok, lp, A, P, STOP, max_dec, mut)
    return [k for k in a if not np.array_equal(a[k], b[k])], a


@pytest.mark.parametrize("T", [1, 70, 128])
def test_tail_emulation_equals_mirror_and_rejects_done_row_writes(T):
    diff, st = book_drive(T, True, True)
    assert diff == [] and st["done"].tolist() == [1, 1, 1, 1, 1, 0] and st["slen"].tolist() == [2, 3, 4, 2, 3, 4]
    assert (st["tok_hist"][3, [0, 1, 3, 4]] == -7777).all() and (st["tok_hist"][3, [2, 5]] != -7777).all()
    diff, _ = book_drive(T, True, True, "tail_done")
    assert {"tok_hist", "lp_sum", "slen", "latest"} <= set(diff)
