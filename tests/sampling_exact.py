"""Exact inputs for the draw kernels of csrc/kernels/sample.hip (helper, no GPU).

Every weight the draw touches is a multiple of 2**-24 not above 1 and the total W is a power of two,
so every fp32 partial sum and u * W are exact whatever the order of the sums: the kernel's pick must
EQUAL ``decode.sampling.draw_full`` / ``draw_topk`` at u = sample_uniform(seed, stream, t).

sample_full rows: logit + bias is one constant on 2**k entries and -inf elsewhere (logits and bias
multiples of 1/16, built from integers), p_gen is 0, 0.5 or 1, the attention values are multiples of
2**-24.  Because the host knows u bit for bit, the weights are laid around it: a prefix sum EQUAL to
u * W (a tie: the pick is the next entry of positive weight, across a run of zero-weight entries), and
the twin whose prefix is 2**-24 higher (the pick is the entry before).  ``full_launches()`` /
``topk_launches()`` list the launches; ``check_full`` / ``check_topk`` assert the conditions on the
float64 reference inputs alone.  ``book_step`` is the plain Python mirror of the bookkeeping tail."""
import functools

import numpy as np

from textsummarization_on_flink_amd.decode.sampling import (draw_full, draw_topk, model_log_prob, sample_uniform)

U = 1 << 24
SEED = 0x5a17ab1e0dd5eed
MIN_DEC, MAX_DEC, STOP = 3, 100, 3
FULL_ROWS, TOPK_ROWS = 392, 468                    # exact rows of full_launches() / topk_launches()
NEG = float("-inf")
_M = np.uint64(0xFFFFFFFF)
# streams whose uniform is exactly 0.5 at SEED (found by search; ``_half_stream`` asserts them): the only
# u at which the prefix of the whole vocabulary part (p_gen = 0.5, W = 1) equals u * W
_HALF = {(2, 0): 3709282, (2, 1 << 33): 8593024062, (3, 0): 15930096, (3, 1 << 33): 8608217418}


def uniforms24(seed, streams, t):
    """sample_uniform * 2**24 of many streams at once (int64)."""
    s = np.asarray(streams, np.uint64)
    c0, c1, c2, c3 = np.full(s.shape, t, np.uint64), s & _M, s >> np.uint64(32), np.zeros_like(s)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return (c0 >> np.uint64(8)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def find_stream(seed, t, base, lo, hi, div):
    """The first stream >= base whose uniform * 2**24 lies in [lo, hi) and is a multiple of div."""
    for s0 in range(base, base + (1 << 25), 1 << 16):
        st = np.arange(s0, s0 + (1 << 16), dtype=np.uint64)
        v = uniforms24(seed, st, t)
        hit = np.nonzero((v >= lo) & (v < hi) & (v % div == 0))[0]
        if len(hit):
            s = int(st[hit[0]])
            assert int(round(sample_uniform(seed, s, t) * U)) == int(v[hit[0]])  # (the scalar host rule agrees)
            return s
    raise AssertionError("no such stream")


def _half_stream(t, base):
    s = _HALF[(t, base)]
    assert sample_uniform(SEED, s, t) == 0.5
    return s


def _compose(rng, total, n):
    """n positive integers that sum to total."""
    assert 0 < n <= total, (n, total)
    return rng.multinomial(total - n, np.full(n, 1.0 / n)).astype(np.int64) + 1


def _pow2(x):
    return x > 0 and x & (x - 1) == 0


# ------------------------------------------------------------------ sample_full
def _row(rng, V, T, L, ext, stop, allow, t, base, sp):
    """One row: (finite vocabulary ids, attention in units of 2**-24 [T], p_gen, stream).
    sp: pg (None: no pointer), k, stop_fin, W (units), tie = None | dict(kind, b, run, delta)."""
    pg, k, tie = sp["pg"], sp["k"], sp.get("tie")
    ptr = pg is not None
    pgu = U if not ptr else int(pg * U)
    assert pgu % (1 << k) == 0
    wv = pgu >> k                                     # weight of a finite vocabulary entry
    nF = 1 << k
    stop_in = 0 <= stop < V and sp.get("stop_fin", True)
    s_masked = stop_in and not allow
    Mv = wv * (nF - s_masked)
    is_stop = np.zeros(T, bool)
    if ptr:
        is_stop[:L] = ext[:L] == stop
    mpos = is_stop & (not allow)                      # positions that weigh 0 whatever their attention
    half = ptr and pg == 0.5
    if not ptr or pg == 1.0:
        W = Mv
    else:
        W = sp.get("W", U // 2 if (s_masked and half) or (pg == 0.0 and mpos.any()) else U)
    assert _pow2(W), (W, Mv)
    P = W - Mv                                        # total of the position weights
    kind = tie["kind"] if tie else None
    lo, hi, div = 0, U, U // W
    # ---- the stream
    if kind == "voc":
        b, run = tie["b"], tie["run"]
        excl = 0 <= stop < V and (s_masked or not stop_in)  # [STOP] is no free finite id
        nb = b + 1 - (excl and stop <= b)             # free ids <= b
        na = V - (b + run + 1) - (excl and stop > b + run)
        jlo, jhi = max(1, (nF - s_masked) - na), min(nb, nF - s_masked - 1)
        assert jlo <= jhi, (jlo, jhi)
        div = wv * U // W
        lo, hi = jlo * div, jhi * div + 1
    elif kind == "pos":
        b, run = tie["b"], tie["run"]
        npos = int((~mpos[:L]).sum())
        margin = npos + 2
        assert P > 2 * margin, (P, margin)
        lo, hi = -(-(Mv + margin) * U // W), (W - margin) * U // W
    if kind == "vp":
        assert Mv * 2 == W and wv > 0
        stream = _half_stream(t, base)
    else:
        stream = find_stream(SEED, t, base, lo, hi, div) if tie else base + sp["r"]
    ui = int(round(sample_uniform(SEED, stream, t) * U))
    assert (ui * W) % U == 0 or not tie
    target = ui * W // U
    # ---- the vocabulary part
    ids = np.arange(V)
    if kind == "voc":
        j = target // wv
        assert j * wv == target
        ok_lo = ids[(ids < b) & ~((ids == stop) & excl)]
        ok_hi = ids[(ids > b + run) & ~((ids == stop) & excl)]
        assert not excl or stop not in (b, b + run + 1)
        fin = np.concatenate([rng.choice(ok_lo, j - 1, replace=False), [b], [b + run + 1],
                              rng.choice(ok_hi[ok_hi > b + run + 1], nF - s_masked - j - 1, replace=False)])
        if s_masked:
            fin = np.concatenate([fin, [stop]])
    else:
        pool = ids[ids != stop] if 0 <= stop < V else ids
        # (the first three ids finite: what a lane that read past V of the row before would pick up)
        head = pool[:min(3, nF - stop_in)]
        fin = np.concatenate([head, rng.choice(pool[len(head):], nF - stop_in - len(head), replace=False)])
        if stop_in:
            fin = np.concatenate([fin, [stop]])
    assert len(set(fin.tolist())) == nF == len(fin)
    # ---- the position part
    A = np.zeros(T, np.int64)
    if ptr:
        A[L:] = U // 4                                # positive attention past the length: never read
        mul = 2 if half else 1                        # w = (1 - p_gen) * a
        live = np.nonzero(~mpos[:L])[0]
        if pg == 1.0:
            A[:L] = rng.integers(0, 1 << 12, L)
        else:
            zero = np.zeros(L, bool)
            if kind in ("pos", "vp"):
                b, run = (tie["b"], tie["run"]) if kind == "pos" else (-1, tie["run"])
                nxt = b + run + 1
                assert nxt < L and not mpos[nxt] and (b < 0 or not mpos[b])
                zero[b + 1:nxt] = True
                free = np.setdiff1d(live, np.arange(max(b, 0), nxt + 1))
                zero[rng.choice(free, len(free) // 8, replace=False)] = True
                hd = live[(live <= b) & ~zero[live]]
                tl = live[(live >= nxt) & ~zero[live]]
                P1 = target - Mv + tie.get("delta", 0)
                if len(hd):
                    A[hd] = _compose(rng, P1, len(hd)) * mul
                else:
                    assert P1 == 0
                A[tl] = _compose(rng, P - P1, len(tl)) * mul
            else:
                zero[rng.choice(live, len(live) // 8, replace=False)] = True
                nz = live[~zero[live]]
                if len(nz):
                    A[nz] = _compose(rng, P, len(nz)) * mul
                else:
                    assert P == 0
            # masked [STOP] copies keep a positive attention (the rest of the mass, where there is some)
            mp = np.nonzero(mpos[:L])[0]
            if len(mp):
                A[mp] = _compose(rng, max(U - int(A[:L].sum()), 4 * len(mp)), len(mp))
            zz = np.nonzero(zero & ~mpos[:L])[0]
            A[zz] = 0
        assert A.max() <= U
    return np.sort(fin), A, pg, stream


def _launch(name, V, T, rows, lens, t, specs, stop=STOP, stop_pos=(), base=0, rseed=0):
    """R = len(specs) rows, ``rows`` per article; lens per article; stop_pos: positions that copy [STOP]."""
    rng = np.random.default_rng([V, T, t, rseed])
    R = len(specs)
    Na = R // rows
    assert Na * rows == R and len(lens) == Na and R <= 8
    allow = t >= MIN_DEC
    ptr = specs[0]["pg"] is not None
    ext = rng.integers(4, V + 40, (Na, T)).astype(np.int32)
    ext[ext == stop] = stop + 1
    for a in range(Na):
        for p in stop_pos:
            if p < T:
                ext[a, p] = stop
        ext[a, lens[a]:] = stop
    bias16 = rng.integers(-32, 33, V)
    c16 = 20                                          # logit + bias = 1.25
    logits = np.full((R, V), NEG, np.float32)
    attn, pgs, streams, want, fins = np.zeros((R, T)), np.ones(R), [], [], []
    for r, sp in enumerate(specs):
        a = r // rows
        fin, A, pg, stream = _row(rng, V, T, lens[a], ext[a], stop, allow, t, base, dict(sp, r=r))
        logits[r, fin] = (c16 - bias16[fin]) / 16.0   # (integers: exact)
        attn[r], streams = A / U, streams + [stream]
        pgs[r] = 1.0 if pg is None else pg
        fins.append(fin)
    bias = (bias16 / 16.0).astype(np.float32)
    L = dict(name=name, V=V, T=T, rows=rows, R=R, lens=np.asarray(lens, np.int32), t=t, stop=stop, ptr=ptr,
             ext=ext, bias=bias, logits=logits, attn=attn.astype(np.float32), pg=pgs.astype(np.float32),
             streams=streams, fins=fins, specs=specs)
    assert (L["attn"].astype(np.float64) == attn).all()
    picks, toks, lps = [], [], []
    for r in range(R):
        vd, a64, pg, e, n = full_reference(L, r)
        ent, tok = draw_full(vd, a64, pg, e, n, sample_uniform(SEED, streams[r], t), stop, allow)
        picks.append(ent)
        toks.append(tok)
        lps.append(model_log_prob(tok, vd, a64, pg, e, n))
    L.update(want_pick=np.asarray(picks), want_tok=np.asarray(toks), want_lp=np.asarray(lps))
    return L


def full_reference(L, r):
    """float64 inputs of ``draw_full`` for row r, from the fp32 arrays the kernel is given."""
    x = L["logits"][r].astype(np.float64) + L["bias"].astype(np.float64)
    e = np.exp(x - x.max())
    vd = e / e.sum()
    a = r // L["rows"]
    return (vd, L["attn"][r].astype(np.float64), float(L["pg"][r]) if L["ptr"] else None, L["ext"][a],
            int(L["lens"][a]))


def full_weights(L, r):
    vd, a64, pg, e, n = full_reference(L, r)
    if pg is None:
        w, toks = vd.copy(), np.arange(L["V"])
    else:
        w, toks = np.concatenate([pg * vd, (1 - pg) * a64[:n]]), np.concatenate([np.arange(L["V"]), e[:n]])
    if L["t"] < MIN_DEC:
        w[toks == L["stop"]] = 0.0
    return w


def check_full(L):
    """The conditions of exactness, on the reference inputs alone; returns per-row tie flags."""
    ties = []
    x = L["logits"].astype(np.float64) + L["bias"].astype(np.float64)
    assert (L["logits"][np.isfinite(L["logits"])] * 16 % 1 == 0).all() and (L["bias"] * 16 % 1 == 0).all()
    for r in range(L["R"]):
        fin = x[r][np.isfinite(x[r])]
        assert len(fin) and (fin == fin[0]).all() and _pow2(len(fin)) and len(fin) < U
        w = full_weights(L, r) * U
        assert (w == np.round(w)).all() and w.min() >= 0 and w.max() <= U
        W = int(w.sum())
        assert _pow2(W) and W <= U, W
        ui = int(round(sample_uniform(SEED, L["streams"][r], L["t"]) * U))
        c = np.cumsum(w)
        if (ui * W) % U == 0:
            ties.append(bool((c == ui * W // U).any()))
        else:
            ties.append(False)
        if L["specs"][r].get("tie"):
            assert ties[-1] == (L["specs"][r]["tie"].get("delta", 0) == 0), (L["name"], r)
    return ties


EXTRA_BASES = (7, (1 << 32) + 11, (1 << 40) + 5)


@functools.lru_cache(maxsize=None)
def _extra(name):
    L = next(x for x in full_launches() if x["name"] == name)
    allow, out = L["t"] >= MIN_DEC, []
    for base in EXTRA_BASES:
        # (u even in units of 2**-24: u * W is exact at W = 1 and W = 1 / 2, the two totals the rows have)
        st = [find_stream(SEED, L["t"], base + 50 * r, 0, U, 2) for r in range(L["R"])]
        pk, tk, lp = [], [], []
        for r in range(L["R"]):
            vd, a64, pg, e, n = full_reference(L, r)
            ent, tok = draw_full(vd, a64, pg, e, n, sample_uniform(SEED, st[r], L["t"]), L["stop"], allow)
            pk.append(ent)
            tk.append(tok)
            lp.append(model_log_prob(tok, vd, a64, pg, e, n))
        out.append(dict(L, streams=st, want_pick=np.asarray(pk), want_tok=np.asarray(tk), want_lp=np.asarray(lp),
                        specs=[{}] * L["R"]))
    return out


def extra_draws(L):
    """The same inputs at three more streams per row (no tie planted): launches with their own expectations."""
    return _extra(L["name"])


def _tie(kind, b=0, run=0, delta=0):
    return dict(kind=kind, b=b, run=run, delta=delta)


def _pair(pg, k, b, run, **kw):
    """a position tie and its twin (prefix 2**-24 higher)"""
    return [dict(pg=pg, k=k, tie=_tie("pos", b, run, 0), **kw), dict(pg=pg, k=k, tie=_tie("pos", b, run, 1), **kw)]


@functools.lru_cache(maxsize=None)
def full_launches():
    """The exact launches of sample_full (sections 1 and 2 of the write-up)."""
    out = []
    B33 = 1 << 33
    for t in (MIN_DEC - 1, MIN_DEC):
        # V = 64, T = 1: one vocabulary chunk, one position; [STOP] = 3 is lane 0's entry
        out.append(_launch(f"v64_t{t}", 64, 1, 1, [1, 1, 1, 1], t,
                           [dict(pg=0.5, k=5), dict(pg=0.0, k=5), dict(pg=1.0, k=5, stop_fin=t >= MIN_DEC),
                            dict(pg=1.0, k=4, stop_fin=False, tie=_tie("voc", 20, 5))]))
        # V = 256, T = 255: [STOP] = 255 is lane 63's entry of the only vocabulary chunk; ties inside the
        # position chunk with the three kinds of zero-weight entry in the run (a = 0, a masked copy at 102)
        out.append(_launch(f"v256_t{t}", 256, 255, 1, [255, 200, 255, 130, 255, 255], t,
                           _pair(0.5, 3, 100, 4) + _pair(0.0, 6, 100, 4) +
                           [dict(pg=0.5, k=7, tie=_tie("voc", 254 - 3, 2), stop_fin=True, W=U),
                            dict(pg=0.5, k=8 if t >= MIN_DEC else 4)],
                           stop=255, stop_pos=(102, 7), base=B33))
        # V = 257: the scalar load path, one entry ([STOP] = 256, lane 0) in the second chunk; T = 256
        out.append(_launch(f"v257_t{t}", 257, 256, 3, [256, 31], t,
                           _pair(0.5, 2, 254, 0) + [dict(pg=1.0, k=7, stop_fin=t >= MIN_DEC)] +
                           [dict(pg=0.5, k=8, stop_fin=False, tie=_tie("pos", 3, 9)), dict(pg=0.0, k=1),
                            dict(pg=0.5, k=5)], stop=256, stop_pos=(5, 9, 200)))
        # V = 3000 (12 chunks), T = 257: a chunk boundary of the position part (entries 255 | 256), the last
        # entry of positive weight, the vocabulary-to-position boundary (u = 0.5), vocabulary ties inside a
        # chunk and on a chunk boundary with -inf runs and the masked [STOP] in them
        out.append(_launch(f"v3000_t{t}", 3000, 257, 1, [257] * 8, t,
                           _pair(0.5, 4, 255, 0) + _pair(0.0, 11, 250, 5) +
                           [dict(pg=0.5, k=4, tie=_tie("pos", 254, 1)),       # the last positive entry: 256
                            dict(pg=0.5, k=11, stop_fin=False, tie=_tie("vp", run=2)),
                            dict(pg=1.0, k=11, stop_fin=t >= MIN_DEC, tie=_tie("voc", 1000, 30)),
                            dict(pg=1.0, k=11, stop_fin=False, tie=_tie("voc", 255, 0))],
                           stop_pos=(1, 252), base=0))
        out.append(_launch(f"v3000s_t{t}", 3000, 512, 3, [512, 300], t,
                           [dict(pg=0.5, k=11, stop_fin=False, tie=_tie("vp", run=1)),
                            dict(pg=0.5, k=3, tie=_tie("voc", 2, 5), W=U),   # [STOP] = 3 in the run (masked at t = 2)
                            dict(pg=0.0, k=2, tie=_tie("pos", 200, 300)),     # a whole zero-weight chunk in the run
                            dict(pg=0.5, k=10), dict(pg=0.0, k=10), dict(pg=0.5, k=4, tie=_tie("pos", 298, 0))],
                           stop_pos=(0, 260), base=B33))
        # V = 3001: the scalar path at 12 chunks; rows after the first start off a 16-byte boundary
        out.append(_launch(f"v3001_t{t}", 3001, 70, 1, [70, 1, 33, 70], t,
                           [dict(pg=1.0, k=11, stop_fin=False, tie=_tie("voc", 2815, 184)),  # next finite id: 3000
                            dict(pg=0.5, k=11, stop_fin=False), dict(pg=0.0, k=11),
                            dict(pg=0.5, k=5, tie=_tie("pos", 30, 2))], stop_pos=(31,), stop=3007))
        # V = 70000 (274 chunks) and T = 2048 (8): 282 chunks, per = 2
        out.append(_launch(f"v70000_t{t}", 70000, 2048, 3, [2048, 700], t,
                           [dict(pg=0.5, k=16, stop_fin=False, tie=_tie("pos", 511, 0)),   # chunks 275 | 276 = 2 * 138
                            dict(pg=0.5, k=16, stop_fin=False, tie=_tie("pos", 511, 0, 1)),
                            dict(pg=1.0, k=16, stop_fin=False, tie=_tie("voc", 256 * 100 - 1, 300)),  # 99 | 100 .. 101
                            dict(pg=0.5, k=16, stop_fin=False, tie=_tie("vp", run=1)),      # chunks 273 | 274 = 2 * 137
                            dict(pg=1.0, k=16, stop_fin=False, tie=_tie("voc", 256 * 101 - 1, 0)),   # 100 | 101: in a segment
                            dict(pg=0.0, k=16, tie=_tie("pos", 690, 5))], stop_pos=(0, 693), base=B33))
        out.append(_launch(f"v70000n_t{t}", 70000, 1, 1, [1, 1, 1], t,
                           [dict(pg=None, k=16, stop_fin=t >= MIN_DEC), dict(pg=None, k=10, stop_fin=False),
                            dict(pg=None, k=16, stop_fin=False, tie=_tie("voc", 256 * 137 - 1, 256))]))
        # V = 140000 (547 chunks) and T = 2048: 555 chunks, per = 3; segment starts at chunks 549 and 552
        out.append(_launch(f"v140000_t{t}", 140000, 2048, 1, [2048, 1500], t,
                           [dict(pg=0.5, k=17, stop_fin=False, tie=_tie("pos", 511, 0)),   # chunks 548 | 549
                            dict(pg=1.0, k=17, stop_fin=False, tie=_tie("voc", 256 * 300 - 1, 700))],  # 299 | 302
                           stop_pos=(600,), stop=140005))
        # (R = 1) the crossing in the last chunk of a segment: position 301 is in chunk 548 of 546 .. 548
        out.append(_launch(f"v140000b_t{t}", 140000, 2048, 1, [2048], t,
                           [dict(pg=0.5, k=17, stop_fin=False, tie=_tie("pos", 300, 0, t - MIN_DEC + 1))], stop=140005))
        # the limit: V = 524288 (2048 chunks), T = 2048: 2056 chunks, per = 9; chunk 2052 = 9 * 228 starts a segment
        out.append(_launch(f"v524288_t{t}", 524288, 2048, 1, [2048, 2047], t,
                           [dict(pg=0.5, k=18, stop_fin=False, tie=_tie("pos", 1023, 0)),  # chunks 2051 | 2052
                            dict(pg=1.0, k=18, stop_fin=False, tie=_tie("voc", 256 * 9 * 100 - 1, 1000))],
                           stop_pos=(1030,), base=B33))
        # (R = 1) position 1004 is in chunk 2051, the last of segment 2043 .. 2051
        out.append(_launch(f"v524288b_t{t}", 524288, 2048, 1, [2048], t,
                           [dict(pg=0.5, k=18, stop_fin=False, tie=_tie("pos", 1000, 3, MIN_DEC - t))],
                           stop_pos=(1002,)))
    return out


# ------------------------------------------------------------------ sample_topk
def _topk_launch(K, k, t, temp, L0, rseed):
    """k + 2 rows with [STOP] at rank 0 .. k and one row without, then rows with -inf candidates at the
    front, in the middle and at the end of the kept set, and a row with a single positive weight."""
    rng = np.random.default_rng([K, k, t, rseed])
    rows = []
    for sr in list(range(k + 1)) + [None]:
        ids = rng.permutation(np.arange(10, 10 + K))
        if sr is not None:
            ids[sr] = STOP
        rows.append((ids, np.full(K, L0)))
    for where in ("front", "middle", "end", "one"):
        ids, lp = rng.permutation(np.arange(10, 10 + K)), np.full(K, L0)
        if k >= 3 or where == "one":
            n = max(1, k // 3)
            if where == "front":
                lp[:n] = NEG
            elif where == "middle":
                lp[k // 2:k // 2 + n] = NEG
            elif where == "end":
                lp[k - n:k + 1] = NEG
            elif k >= 2:
                lp[:k + 1] = NEG
                lp[int(rng.integers(0, k))] = L0
        rows.append((ids, lp))
    R = len(rows)
    ids = np.stack([x[0] for x in rows]).astype(np.int32)
    lp = np.stack([x[1] for x in rows]).astype(np.float32)
    lp[:, k + 1:] = rng.integers(-80, -40, (R, K - k - 1)) / 8.0  # (never read: finite junk past the k + 1 best)
    # (u a multiple of 2**-19: u * W, W <= 31, then has at most 24 bits and the fp32 product rounds nothing)
    streams = [find_stream(SEED, t, (1 << 32) * (r % 3) + 10000 * rseed + 100 * r, 0, U, 32) for r in range(R)]
    return dict(name=f"K{K}_k{k}_t{t}_temp{temp}_L{L0}", K=K, k=k, t=t, temp=temp, R=R, ids=ids, lp=lp,
                streams=streams)


def check_topk(L):
    """Conditions on the reference inputs alone, and the expected picks: weights exactly 1 or 0, the fp32
    target u * W exact (one rounding that rounds nothing)."""
    want = []
    for r in range(L["R"]):
        ids, lp, k = L["ids"][r], L["lp"][r].astype(np.float64), L["k"]
        allow = L["t"] >= MIN_DEC
        cand = [j for j in range(k + 1) if allow or int(ids[j]) != STOP][:k]
        m = lp[cand].max()
        w = np.exp((lp[cand] - m) / L["temp"])
        assert np.isfinite(m) and set(w.tolist()) <= {0.0, 1.0}
        u = sample_uniform(SEED, L["streams"][r], L["t"])
        W = w.sum()
        assert float(np.float32(u) * np.float32(W)) == u * W  # the kernel's target is the host's
        want.append(draw_topk(ids, L["lp"][r], k, L["temp"], u, STOP, allow))
        # (the host rule on exp(lp / temp) in float64 decides as the exact 0 / 1 weights do)
        assert want[-1] == cand[int(np.nonzero((np.cumsum(w) > u * W) & (w > 0))[0][0])]
    return np.asarray(want)


@functools.lru_cache(maxsize=None)
def topk_launches():
    out = []
    for i, (K, k) in enumerate([(2, 1), (4, 3), (9, 8), (32, 31), (32, 5)]):
        for t in (MIN_DEC - 1, MIN_DEC):
            for temp, L0 in ((0.05, 0.0), (1.0, -1.5), (50.0, 0.0)):
                out.append(_topk_launch(K, k, t, temp, L0, i))
    return out


# ------------------------------------------------------------------ the bookkeeping tail
def book_state(R, T, max_dec, att, pg):
    """The books as the tests prefill them (sentinels: -7777 / 12288.0); lp_sum, slen, latest, done start live."""
    st = dict(tok_hist=np.full((max_dec, R), -7777, np.int32), lp_hist=np.full((max_dec, R), 12288.0, np.float32),
              lp_sum=np.zeros(R, np.float32), latest=np.full(R, 2, np.int32), slen=np.zeros(R, np.int32),
              done=np.zeros(R, np.int32))
    if att:
        st["att_hist"] = np.full((max_dec, R, T), 12288.0, np.float32)
    if pg:
        st["pg_hist"] = np.full((max_dec, R), 12288.0, np.float32)
    return st


def book_step(st, t, tok, lp, att, pg, stop, max_dec):
    """sample_book in plain Python: rows done before the step, t < 0 and t >= max_dec change nothing."""
    if t < 0 or t >= max_dec:
        return
    for r in range(len(st["done"])):
        if st["done"][r]:
            continue
        st["tok_hist"][t, r], st["lp_hist"][t, r] = tok[r], lp[r]
        st["lp_sum"][r] = np.float32(st["lp_sum"][r] + np.float32(lp[r]))
        st["latest"][r], st["slen"][r] = tok[r], t + 1
        if tok[r] == stop:
            st["done"][r] = 1
        if "att_hist" in st:
            st["att_hist"][t, r] = att[r]
        if "pg_hist" in st:
            st["pg_hist"][t, r] = pg[r]
