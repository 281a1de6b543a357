"""Op-level tests of the one-wave beam bookkeeping (beam_step, beam_step_ng, beam_step_pen: beam.hip
/ beam_common.h), of the beam tail fused into the vocab select kernel (vocab_topk_beam, _ng, _pen)
and of cov_penalty, against the sequential fp32 mirror of tests/beam_mirror.py (float64 for
cov_penalty).  Every output is a view inside a sentinel allocation (NaN / -7777) compared bit for
bit, the state buffers are prefilled with the same sentinels, and the mirror's state carries them
too: "equal to the mirror" covers what must NOT be written (res_* past the count, history rows
past t, seq past t + 2).  Sums are exact (log-probs are multiples of 2^-10, or of 1/4), the build
divides fp32 correctly rounded (no fast-math flag; hipcc's default), so everything is bit-equal,
res_score = tot / (t + 2) included.  profiles/beam_op_tests.md holds the case table."""
import numpy as np
import pytest
import torch

import beam_mirror as M
from beam_mirror import BETA, ISENT, MAX_DEC, MIN_DEC, STOP, T_ATT, f32

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD = 32
I32, F32, I64, BF = torch.int32, torch.float32, torch.int64, torch.bfloat16


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


class Arena:
    """named contiguous views inside one sentinel allocation (PAD elements before, between and behind them,
    views 16-byte aligned); host() brings the whole allocation back in one copy and checks the sentinels"""

    def __init__(self, arrays):
        self.dtype = next(iter(arrays.values())).dtype
        self.sent = np.array(np.nan if self.dtype == np.float32 else ISENT, self.dtype)
        self.off, o = {}, PAD
        for nm, v in arrays.items():
            assert v.dtype == self.dtype
            self.off[nm] = (o, v.size, v.shape)
            o = (o + v.size + PAD + 3) & ~3
        host = np.full(o, self.sent, self.dtype)
        self.mask = np.ones(o, bool)
        for nm, v in arrays.items():
            b, n, _ = self.off[nm]
            host[b:b + n] = v.ravel()
            self.mask[b:b + n] = False
        self.flat = torch.from_numpy(host).to(DEV)
        self.v = {nm: self.flat[b:b + n].view(*s) for nm, (b, n, s) in self.off.items()}

    def host(self, tag):
        h = self.flat.cpu().numpy()
        hb, sb = h.view(np.int32) if self.dtype == np.float32 else h, self.sent.view(np.int32) if self.dtype == np.float32 else self.sent
        bad = np.nonzero(self.mask & (hb != sb))[0]
        assert bad.size == 0, "%s: sentinel: %d elements outside the views changed, first at %d (%r)" % (tag, bad.size, bad[0], self.off)
        return {nm: h[b:b + n].reshape(s) for nm, (b, n, s) in self.off.items()}


class DevState:
    """the bookkeeping state of beam_mirror on the device: one float and one int arena"""

    def __init__(self, st, hist_T=0):
        fa = {k: st[k] for k in ("lp", "key", "rs", "rlp")}
        ia = {k: st[k] for k in ("latest", "gidx", "th", "ph", "done", "rc", "rl", "rst", "rp", "step", "ctr", "seq0", "seq1")}
        maxD, R = st["th"].shape
        if hist_T:
            fa["ah"], fa["pgh"] = np.full((maxD, R, hist_T), np.nan, f32), np.full((maxD, R), np.nan, f32)
        self.f, self.i = Arena(fa), Arena(ia)
        self.v = {**self.f.v, **self.i.v}

    def host(self, tag):
        return {**self.f.host(tag), **self.i.host(tag)}

    def clone(self):
        c = object.__new__(DevState)
        c.f, c.i = object.__new__(Arena), object.__new__(Arena)
        for src, dst in ((self.f, c.f), (self.i, c.i)):
            dst.__dict__.update(src.__dict__)
            dst.flat = src.flat.clone()
            dst.v = {nm: dst.flat[b:b + n].view(*s) for nm, (b, n, s) in src.off.items()}
        c.v = {**c.f.v, **c.i.v}
        return c

    def same_bits(self, other):
        return torch.equal(self.f.flat.view(I32), other.f.flat.view(I32)) and torch.equal(self.i.flat, other.i.flat)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def call_beam_step(k, ds, ids, lps, t, Na, beam, K, min_dec, max_dec, n, pen, use_ctr, att=None, pg=None):
    """the op of the option set: beam_step (plain), beam_step_ng (n > 1), beam_step_pen (penalties, with or without n)"""
    v = ds.v
    if not use_ctr:
        v["step"].fill_(t + 1)  # the caller advanced the counter at the start of the decode step
    hist = att is not None and "ah" in v
    args = [_dev(ids), _dev(lps), v["lp"], v["latest"], v["gidx"], v["th"], v["ph"], v["done"], v["rc"], v["rs"], v["rl"],
            v["rst"], v["rp"], v["step"], v["ctr"] if use_ctr else None, _dev(att) if hist else None,
            v["ah"] if hist else None, _dev(pg) if hist else None, v["pgh"] if hist else None, T_ATT, Na, beam, K, STOP,
            min_dec, max_dec]
    if pen:
        k.beam_step_pen(*args, v["seq0"] if n > 1 else None, v["seq1"] if n > 1 else None, n, _dev(pen[0]), _dev(pen[2]),
                        pen[1], v["key"], v["rlp"])
    elif n > 1:
        k.beam_step_ng(*args, v["seq0"], v["seq1"], n)
    else:
        k.beam_step(*args)


# ------------------------------------------------------------------ b. beam_step* against the mirror
def _run_drive(k, d, use_ctr, hist):
    ds = DevState(d.init, T_ATT if hist else 0)
    exp_ah, exp_pgh = np.full((MAX_DEC, d.Na * d.beam, T_ATT), np.nan, f32), np.full((MAX_DEC, d.Na * d.beam), np.nan, f32)
    names = d.names(use_ctr)
    for s in d.steps:
        t = s["t"]
        tag = "beam %d K %d Na %d %s ctr=%s hist=%s t=%d" % (d.beam, d.K, d.Na, d.mode, use_ctr, hist, t)
        call_beam_step(k, ds, s["ids"], s["lps"], t, d.Na, d.beam, d.K, MIN_DEC, MAX_DEC, d.n, d.pen(s["cpen"]), use_ctr,
                       s["att"] if hist else None, s["pg"])
        got = ds.host(tag)
        M.assert_state(tag, got, s["exp"], names)
        if hist:  # row min(t, max_dec - 1): the call at t = max_dec overwrites the last row
            exp_ah[min(t, MAX_DEC - 1)], exp_pgh[min(t, MAX_DEC - 1)] = s["att"], s["pg"]
            assert np.array_equal(got["ah"].view(np.int32), exp_ah.view(np.int32)), tag + ": [att_hist]"
            assert np.array_equal(got["pgh"].view(np.int32), exp_pgh.view(np.int32)), tag + ": [pg_hist]"
    # the last step was the call at t = max_dec: identity gidx and nothing else (the mirror's state says so)
    assert got["gidx"].tolist() == list(range(d.Na * d.beam))


@pytest.mark.parametrize("Na", M.NAS)
@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("beam,K", M.SHAPES)
def test_beam_step_matches_mirror(beam, K, mode, Na):
    """12 steps from t = 0 and the call at t = max_dec, state carried on the device, against the
    mirror at every step: once with ctr (the kernel advances step and leaves ctr at 0) and the
    histories, once with ctr = None (the caller sets step = t + 1) and no histories."""
    k = _ops()
    d = M.Drive(beam, K, Na, mode)
    assert not d.conditions(), d.conditions()
    _run_drive(k, d, True, True)
    _run_drive(k, d, False, False)


@pytest.mark.parametrize("use_ctr", [True, False])
@pytest.mark.parametrize("form", ["plain", "ng", "pen"])
def test_beam_step_mid_run_at_the_ban_table_limit(form, use_ctr):
    """one step entered at t = 250 with beam * P = NG_BAN_MAX (beam_mirror.MidRun)"""
    k = _ops()
    m = M.MidRun(form)
    st = M.copy_state(m.init)
    ds = DevState(st, T_ATT)
    mm = M.MID
    call_beam_step(k, ds, m.ids, m.lps, m.t, m.Na, m.beam, m.K, mm["min_dec"], mm["max_dec"], m.n, m.pen(m.cpen), use_ctr,
                   m.att, m.pg)
    tag = "mid-run %s ctr=%s" % (form, use_ctr)
    got = ds.host(tag)
    M.assert_state(tag, got, m.exp, m.names(use_ctr))
    assert np.array_equal(got["ah"][m.t], m.att) and np.array_equal(got["pgh"][m.t], m.pg)
    assert np.isnan(got["ah"][:m.t]).all() and np.isnan(got["ah"][m.t + 1:]).all() and np.isnan(got["pgh"][m.t + 1:]).all()


# ------------------------------------------------------------------ c. the fused tail
V, T_F, A_MUL, E_F = 600, 24, 2, 32
F_STEPS, F_MAXD, F_P = 8, 10, 12
POOL = 10 + np.arange(5)


def _bf(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(BF)


class HeadInputs:
    """per-step inputs of the vocab head for R rows: logits peaked on 5 ids (the beams revisit tokens, so bigrams
    repeat), [STOP] raised per article and step with probability PSTOP[a % 6] (a single article: 0.15) and lowered
    otherwise, in-article OOV ids >= V in ext, attention over lens[a] positions"""

    def __init__(self, H, Na, beam, seed, tie_article=None):
        self.H, self.Na, self.beam, self.R = H, Na, beam, Na * beam
        self.A, self.E = A_MUL * H, E_F
        self.rng = rng = np.random.default_rng([seed, H, Na, beam])
        self.u = rng.choice([-1.0, 1.0], H).astype(f32)
        W = (rng.standard_normal((V, H)) * H ** -0.5).astype(f32)
        W[STOP] = self.u * 0.5
        self.WT = _bf(W).to(DEV)
        self.bias0 = (rng.standard_normal(V) * 0.3).astype(f32)
        self.bias0[POOL] += 5.0
        self.lens = rng.integers(T_F // 2, T_F + 1, Na).astype(np.int32)
        self.lens[0] = T_F
        self.ext = rng.integers(4, V + 6, (Na, T_F)).astype(np.int32)
        self.ext[:, :4] = rng.integers(V, V + 6, (Na, 4))
        self.pg_w = (rng.standard_normal(self.A + 2 * H + self.E) * 0.05).astype(f32)
        self.pg_b = np.array([0.3], f32)
        self.tie_article = tie_article
        self.d = dict(WT=self.WT, ext=_dev(self.ext), lens=_dev(self.lens), pg_w=_dev(self.pg_w), pg_b=_dev(self.pg_b))

    def step(self):
        rng, R, H, beam = self.rng, self.R, self.H, self.beam
        X = (rng.standard_normal((R, H)) * 0.7).astype(f32)
        for a in range(self.Na):
            p = 0.15 if self.Na == 1 else M.PSTOP[a % 6]
            boost = 16.0 if rng.random() < p else -16.0          # logit of [STOP] moves by boost (u . u = H)
            X[a * beam:(a + 1) * beam] += boost / (0.5 * H) * self.u
        attn = rng.random((R, T_F)).astype(f32)
        attn *= np.arange(T_F)[None] < np.repeat(self.lens, beam)[:, None]
        attn = (attn / attn.sum(1, keepdims=True)).astype(f32)
        ctx, c, x = (rng.standard_normal((R, n)).astype(f32) for n in (self.A, H, self.E))
        h = rng.standard_normal((R, H)).astype(f32)
        if self.tie_article is not None:  # identical operands on all rows of one article
            sl = slice(self.tie_article * beam, (self.tie_article + 1) * beam)
            for v in (X, attn, ctx, c, x, h):
                v[sl] = v[sl.start]
        return dict(X=_bf(X).to(DEV), bias=_dev(self.bias0), attn=_dev(attn), ctx=_dev(ctx), c=_dev(c), h=_bf(h).to(DEV),
                    x=_dev(x), cpen=(rng.integers(0, 256, R) / 64.0).astype(f32), attn_host=attn)


def _head_out(R, K, nt):
    return Arena({"lp": np.full((R, K), np.nan, f32), "lg": np.full((R, V), np.nan, f32), "ms": np.full((R, nt, 2), np.nan, f32),
                  "pgo": np.full(R, np.nan, f32)}), Arena({"ids": np.full((R, K), ISENT, np.int32)})


def call_fused(k, hi, s, ds, of, oi, aux, K, ptr, hist, n, pen, min_dec=MIN_DEC, max_dec=F_MAXD):
    v, d, R = ds.v, hi.d, hi.R
    args = [s["X"], d["WT"], s["bias"]] + ([s["ctx"], s["c"], s["h"], s["x"], d["pg_w"], d["pg_b"], of.v["pgo"]] if ptr else [None] * 7)
    args += [s["attn"] if (ptr or hist) else None, d["ext"], d["lens"], oi.v["ids"], of.v["lp"], of.v["lg"], of.v["ms"], v["lp"], v["latest"],
             v["gidx"], v["th"], v["ph"], v["done"], v["rc"], v["rs"], v["rl"], v["rst"], v["rp"], v["step"], aux["art_ctr"],
             aux["gran"], aux["err"], v["ah"] if hist else None, v["pgh"] if (hist and ptr) else None, R, V, hi.H, T_F, K, hi.beam,
             hi.A, hi.E, STOP, min_dec, max_dec]
    if pen:
        k.vocab_topk_beam_pen(*args, v["seq0"] if n > 1 else None, v["seq1"] if n > 1 else None, n, _dev(pen[0]), _dev(pen[2]),
                              pen[1], v["key"], v["rlp"])
    elif n > 1:
        k.vocab_topk_beam_ng(*args, v["seq0"], v["seq1"], n)
    else:
        k.vocab_topk_beam(*args)


def call_head(k, hi, s, of, oi, K, ptr):
    d, R = hi.d, hi.R
    if ptr:
        k.vocab_topk_pg(s["X"], d["WT"], s["bias"], s["ctx"], s["c"], s["h"], s["x"], d["pg_w"], d["pg_b"], of.v["pgo"], s["attn"],
                        d["ext"], d["lens"], oi.v["ids"], of.v["lp"], of.v["lg"], of.v["ms"], R, V, hi.H, T_F, K, hi.beam, hi.A, hi.E)
    else:
        k.vocab_topk(s["X"], d["WT"], s["bias"], None, None, d["ext"], d["lens"], oi.v["ids"], of.v["lp"], of.v["lg"], of.v["ms"], R, V,
                     hi.H, T_F, K, hi.beam)


def _aux(R, Na, K, stale_step=None):
    """art_ctr, err (zero) and the granules: zero, or stale -- the tag of the step before and a payload (log-prob
    1000, id 9) that would win every rank"""
    g = torch.zeros(R * K, dtype=I64, device=DEV)
    if stale_step is not None:
        g.fill_((((stale_step & 0x7fff) << 17 | 9) << 32) | int(np.array(1000.0, f32).view(np.uint32)))
    ia = Arena({"art_ctr": np.zeros(Na, np.int32), "err": np.zeros(1, np.int32)})
    return {"art_ctr": ia.v["art_ctr"], "err": ia.v["err"], "gran": g, "arena": ia}


def _fused_step(k, hi, s, t, ds, exp, K, ptr, hist, n, pen_of, stale, kind, tag, exp_hist):
    """one decode step through the fused op with every check of the step; returns the counters of the mirror"""
    R, Na, beam = hi.R, hi.Na, hi.beam
    nt = int(k.vocab_topk_parts(V, hi.H))
    aux = _aux(R, Na, K, t if stale else None)  # step = t + 1: the stale tag is t
    pre = ds.clone()
    of, oi = _head_out(R, K, nt)
    rf, ri = _head_out(R, K, nt)
    ds.v["step"].fill_(t + 1)
    pen = pen_of(s["cpen"])
    call_fused(k, hi, s, ds, of, oi, aux, K, ptr, hist, n, pen)
    call_head(k, hi, s, rf, ri, K, ptr)
    o, r = {**of.host(tag), **oi.host(tag)}, {**rf.host(tag), **ri.host(tag)}
    for nm in ("ids", "lp", "lg") + (("pgo",) if ptr else ()):
        assert np.array_equal(M._bits(o[nm]), M._bits(r[nm])), "%s: [%s] differs from vocab_topk%s" % (tag, nm, "_pg" if ptr else "")
    assert not np.isnan(o["lp"]).any() and (o["ids"] >= 0).all() and (o["ids"] < V + T_F).all(), tag
    a = aux["arena"].host(tag)
    assert not a["art_ctr"].any(), tag + ": [art_ctr] not back at zero"
    assert a["err"][0] == 0, tag + ": [err] the poll timed out"
    want = (np.int64((t + 1) & 0x7fff) << 49) | (o["ids"].astype(np.int64) << 32) | o["lp"].view(np.uint32).astype(np.int64)
    assert np.array_equal(aux["gran"].cpu().numpy().reshape(R, K), want), tag + ": [gran]"
    cnt = M.mirror_step(exp, o["ids"], o["lp"], t, beam, K, STOP, MIN_DEC, F_MAXD, n, pen)
    exp["step"][0] = t + 1
    names = M.state_names(n, bool(pen), False) + ["ctr"]
    got = ds.host(tag)
    M.assert_state(tag, got, exp, names)
    if hist:
        exp_hist[0][t] = s["attn_host"]
        assert np.array_equal(got["ah"].view(np.int32), exp_hist[0].view(np.int32)), tag + ": [att_hist]"
        if ptr:
            exp_hist[1][t] = o["pgo"]
            assert np.array_equal(got["pgh"].view(np.int32), exp_hist[1].view(np.int32)), tag + ": [pg_hist]"
        else:
            assert np.isnan(got["pgh"]).all(), tag + ": [pg_hist] written without the pointer inputs"
    # the separate op from the state before the step: the whole allocation, sentinels included, bit for bit
    call_beam_step_f(k, pre, o["ids"], o["lp"], t, Na, beam, K, n, pen, s["attn_host"] if hist else None,
                     o["pgo"] if (hist and ptr) else None)
    assert ds.same_bits(pre), tag + ": [beam_step] the fused tail and the separate op differ"
    return cnt


def call_beam_step_f(k, ds, ids, lps, t, Na, beam, K, n, pen, att, pg):
    v = ds.v
    v["step"].fill_(t + 1)
    args = [_dev(ids), _dev(lps), v["lp"], v["latest"], v["gidx"], v["th"], v["ph"], v["done"], v["rc"], v["rs"], v["rl"], v["rst"],
            v["rp"], v["step"], None, _dev(att) if att is not None else None, v["ah"] if att is not None else None,
            _dev(pg) if pg is not None else None, v["pgh"] if pg is not None else None, T_F, Na, beam, K, STOP, MIN_DEC, F_MAXD]
    if pen:
        k.beam_step_pen(*args, v["seq0"] if n > 1 else None, v["seq1"] if n > 1 else None, n, _dev(pen[0]), _dev(pen[2]), pen[1],
                        v["key"], v["rlp"])
    elif n > 1:
        k.beam_step_ng(*args, v["seq0"], v["seq1"], n)
    else:
        k.beam_step(*args)


def _fused_opts(kind):
    """(n, penalties) of the op: plain, _ng (bigram blocking), _pen (penalties, with bigram blocking in the
    pointer drive and without in the baseline drive: both instantiations of the select kernel with a BeamPen)"""
    return {"plain": (0, False), "ng": (2, False), "pen": (2, True)}[kind]


def _inv_len():
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.decode.beam_search import inv_len_table
    return inv_len_table(HParams(length_penalty="wu", length_alpha=0.9), F_MAXD + 1)


def _fused_drive(k, H, beam, K, Na, kind, ptr, hist, stale, seed=0, n=None):
    n, use_pen = (_fused_opts(kind)[0] if n is None else n), _fused_opts(kind)[1]
    hi = HeadInputs(H, Na, beam, seed)
    exp = M.new_state(Na, beam, F_MAXD, F_P)
    ds = DevState(exp, T_F)
    inv = _inv_len()
    pen_of = (lambda cp: (inv, BETA, cp)) if use_pen else (lambda cp: None)
    exp_hist = (np.full((F_MAXD, hi.R, T_F), np.nan, f32), np.full((F_MAXD, hi.R), np.nan, f32))
    tot = dict(blocked=0, results=0)
    for t in range(F_STEPS):
        tag = "fused %s H %d beam %d K %d Na %d ptr=%s hist=%s stale=%s t=%d" % (kind, H, beam, K, Na, ptr, hist, stale, t)
        c = _fused_step(k, hi, hi.step(), t, ds, exp, K, ptr, hist, n, pen_of, stale, kind, tag, exp_hist)
        for nm in tot:
            tot[nm] += c[nm]
    return tot


FUSED_SHAPES = [(1, 2), (2, 4), (3, 6), (4, 8), (8, 8)]


@pytest.mark.parametrize("Na", [1, 3, 40])
@pytest.mark.parametrize("kind", ["plain", "ng", "pen"])
@pytest.mark.parametrize("beam,K", FUSED_SHAPES)
@pytest.mark.parametrize("H", [128, 64])
def test_fused_tail_matches_head_mirror_and_separate_op(H, beam, K, kind, Na):
    """8 decode steps with the state carried, two drives per case so that the pointer / baseline form, the
    histories and the stale / zero granules each appear on and off with every kernel, width and shape: (pointer,
    one of histories / no histories, stale granules) and (baseline, the other, zero granules)."""
    k = _ops()
    flip = (FUSED_SHAPES.index((beam, K)) + (H == 64) + [1, 3, 40].index(Na)) % 2 == 1
    a = _fused_drive(k, H, beam, K, Na, kind, True, not flip, True)
    b = _fused_drive(k, H, beam, K, Na, kind, False, flip, False, seed=1, n=0 if kind == "pen" else None)
    if Na > 1:  # the drive reached results (the mirror's counters)
        assert a["results"] + b["results"] > 0, (a, b)
    if Na == 40 and kind != "plain" and beam > 1:  # and, with 40 articles' beams over 5 likely tokens, blocked candidates
        assert a["blocked"] > 0, (a, b)


@pytest.mark.parametrize("kind", ["plain", "pen"])
def test_fused_tail_ties_across_hypotheses(kind):
    """one article (of three) whose beam rows have identical X, p_gen operands and attention rows and equal lp_sum:
    its candidates tie pairwise across the hypotheses and the stable candidate order decides; entered at t = 3"""
    k = _ops()
    H, beam, K, Na, t = 128, 4, 8, 3, 3
    n, use_pen = 0, kind == "pen"
    hi = HeadInputs(H, Na, beam, 7, tie_article=1)
    exp = M.new_state(Na, beam, F_MAXD, F_P)
    exp["lp"][:] = f32(-1.5)
    exp["key"][:] = 0
    ds = DevState(exp, T_F)
    inv = _inv_len()
    s = hi.step()
    s["cpen"][beam:2 * beam] = s["cpen"][beam]
    exp_hist = (np.full((F_MAXD, hi.R, T_F), np.nan, f32), np.full((F_MAXD, hi.R), np.nan, f32))
    pen_of = (lambda cp: (inv, BETA, cp)) if use_pen else (lambda cp: None)
    before = M.copy_state(exp)
    _fused_step(k, hi, s, t, ds, exp, K, True, True, n, pen_of, True, kind, "fused ties " + kind, exp_hist)
    # the tie decided: the article's new hypotheses all descend from candidates with equal keys, taken in candidate order
    par = exp["ph"][t, beam:2 * beam].tolist()
    assert par == sorted(par) and len(set(exp["lp"][beam:2 * beam].tolist())) < beam, (par, exp["lp"][beam:2 * beam], before["lp"][0])


def test_fused_tail_graph_replay_equals_eager():
    """the fused op captured with torch.cuda.graph (the counter advance inside the graph) and replayed for two steps
    on fixed inputs == two eager steps"""
    k = _ops()
    H, beam, K, Na = 128, 4, 8, 3
    hi = HeadInputs(H, Na, beam, 11)
    s = hi.step()
    nt = int(k.vocab_topk_parts(V, H))
    out = []
    for graph in (False, True):
        ds = DevState(M.new_state(Na, beam, F_MAXD, F_P), T_F)
        aux = _aux(hi.R, Na, K)
        of, oi = _head_out(hi.R, K, nt)

        def step():
            ds.v["step"].add_(1)
            call_fused(k, hi, s, ds, of, oi, aux, K, True, True, 0, None)

        if graph:
            keep = (ds.f.flat.clone(), ds.i.flat.clone(), aux["gran"].clone())
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()  # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            ds.f.flat.copy_(keep[0]); ds.i.flat.copy_(keep[1]); aux["gran"].copy_(keep[2])
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            ds.f.flat.copy_(keep[0]); ds.i.flat.copy_(keep[1]); aux["gran"].copy_(keep[2])
            g.replay()
            g.replay()
        else:
            step()
            step()
        torch.cuda.synchronize()
        assert int(aux["err"].item()) == 0 and int(ds.v["step"].item()) == 2
        out.append((ds.f.flat.view(I32).cpu(), ds.i.flat.cpu(), aux["gran"].cpu(), oi.flat.cpu(), of.flat.view(I32).cpu()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ d. cov_penalty at its edges
@pytest.mark.parametrize("a0", [False, True])
@pytest.mark.parametrize("R,beam", [(1, 1), (5, 1), (5, 5), (7, 1)])
@pytest.mark.parametrize("T,offset", [(8, 0), (132, 0), (7, 1), (131, 3)])
def test_cov_penalty_edges(T, offset, R, beam, a0):
    """R = 1, 5, 7 rows (a partial 4-row workgroup), beam 1 and 5, with and without a0; lens cycle over T, 1 and 5 (one
    past a float4 edge); offset: cov / att are views at an odd element offset of their allocation (T % 4 != 0: the
    scalar path).  Inputs are multiples of 2^-20 below 2, so every term is exact and only the sum rounds: at most
    len - 1 roundings of relative 2^-24 each over non-negative terms, bound T * 2^-23 * sum.  A second set of inputs in
    multiples of 2^-10 (terms and every partial sum exact below 2^14) must come out bit-equal."""
    k = _ops()
    Na = R // beam
    rng = np.random.default_rng([T, R, beam, int(a0)])
    lens = np.array([(T, 1, 5)[a % 3] for a in range(Na)], np.int32)
    rows = np.repeat(lens, beam)
    for shift, exact in ((20, False), (10, True)):
        one = 1 << shift
        cov = (rng.integers(0, 3 * one // 2, (R, T)) / float(one)).astype(f32)
        att = (rng.integers(0, one // 2, (R, T)) / float(one)).astype(f32)
        z = (rng.integers(0, one // 4, (Na, T)) / float(one)).astype(f32)
        for r in range(R):
            cov[r, rows[r]:], att[r, rows[r]:] = 40.0 + r, np.nan  # past the length: never read into the sum
        z[:, :] = np.where(np.arange(T)[None] < lens[:, None], z, np.nan)

        def place(x):
            flat = torch.full((offset + x.size + PAD,), float("nan"), device=DEV)
            flat[offset:offset + x.size] = _dev(x).flatten()
            return flat[offset:offset + x.size].view(*x.shape)

        out = Arena({"cpen": np.full(R, np.nan, f32)})
        k.cov_penalty(place(cov), place(att), _dev(lens), out.v["cpen"], R, T, beam, place(z) if a0 else None)
        got = out.host("cov_penalty")["cpen"]
        want = np.array([np.maximum(cov[r, :rows[r]].astype(np.float64) + att[r, :rows[r]]
                                    - (z[r // beam, :rows[r]] if a0 else 0.0) - 1.0, 0).sum() for r in range(R)])
        assert np.isfinite(got).all(), got
        if exact:
            assert np.array_equal(got.astype(np.float64), want), (got, want)
        else:
            assert (np.abs(got.astype(np.float64) - want) <= T * 2.0 ** -23 * want).all(), (got, want)
        assert T < 100 or (want[rows == T] > 0).all()  # the full-length rows have something to sum


# ------------------------------------------------------------------ e. what the bindings refuse
def _step_args(Na, beam, K, maxD=4, T=7, P=8, att=False, pg=False):
    R = Na * beam
    zi = lambda *s: torch.zeros(*s, dtype=I32, device=DEV)  # noqa: E731
    zf = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    return [zi(R, K), zf(R, K), zf(R), zi(R), zi(R), zi(maxD, R), zi(maxD, R), zi(Na), zi(Na), zf(R), zi(R), zi(R), zi(R), zi(1),
            None, zf(R, T) if att else None, None, zf(R) if pg else None, None, T, Na, beam, K, STOP, 1, maxD], zi, zf


def test_beam_step_bindings_refuse():
    k = _ops()
    for beam, K in ((5, 13), (1, 17)):  # beam * K = 65; K = 17
        args, _, _ = _step_args(2, beam, K)
        with pytest.raises(RuntimeError, match="bad beam args"):
            k.beam_step(*args)
    beam, K, Na, maxD = 4, 8, 2, 4
    R = Na * beam
    args, zi, zf = _step_args(Na, beam, K)
    for P, same, what in ((6, False, "P % 4"), (4, False, "P < max_dec + 1"), (1028, False, "beam * P > 4096"), (8, True, "seq0 is seq1")):
        s0 = zi(R, P)
        with pytest.raises(RuntimeError, match="seq"):
            k.beam_step_ng(*args, s0, s0 if same else zi(R, P), 3)
    with pytest.raises(RuntimeError, match="inv_len"):  # one short of max_dec + 2
        k.beam_step_pen(*args, None, None, 0, zf(maxD + 1), zf(R), 0.5, zf(R), zf(R))
    with pytest.raises(RuntimeError, match="beta"):
        k.beam_step_pen(*args, None, None, 0, zf(maxD + 2), zf(R), -0.5, zf(R), zf(R))
    with pytest.raises(RuntimeError, match="pairs"):  # att without att_hist
        k.beam_step(*_step_args(Na, beam, K, att=True)[0])
    a = _step_args(Na, beam, K, pg=True)[0]
    a[18] = zf(maxD, R)  # pg and pg_hist, no att
    with pytest.raises(RuntimeError, match="pairs"):
        k.beam_step(*a)
    with pytest.raises(RuntimeError, match="at most 33 argument"):  # the wide entry has no place for a ctr
        k.beam_step_wide(*args[:14], zi(1), *args[15:], None, None, 0, None, None, 0.0, None, None)


@pytest.mark.parametrize("beam,K", [(2, 9), (9, 8)])
def test_fused_bindings_refuse(beam, K):
    """fused K = 9, fused beam * K = 72"""
    k = _ops()
    H, Na = 128, 1
    hi = HeadInputs(H, Na, beam, 3)
    s = hi.step()
    ds = DevState(M.new_state(Na, beam, F_MAXD, F_P), T_F)
    of, oi = _head_out(hi.R, K, int(k.vocab_topk_parts(V, H)))
    with pytest.raises(RuntimeError, match="bad vocab_topk_beam args"):
        call_fused(k, hi, s, ds, of, oi, _aux(hi.R, Na, K), K, True, False, 0, None)
