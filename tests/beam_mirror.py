"""One sequential fp32 mirror of the beam bookkeeping (reference beam_search.py:110-156) for Na
articles with every option, the drives of tests/test_gpu_beam_ops.py, and the named state checks.
No GPU here: tests/test_beam_ops_checks.py runs the same drives and checks on the CPU.

State: a dict of numpy arrays laid out like the device buffers (R = Na * beam rows)

    lp, key      f32 [R]        raw log-prob sum / rank key of each live hypothesis (lp_sum, key_sum)
    latest, gidx i32 [R]        token of each new hypothesis, global row of its parent
    th, ph       i32 [maxD][R]  token / parent history, row t written at step t
    done, rc     i32 [Na]       article finished, results so far
    rs, rlp      f32 [R]        res_score, res_lp (penalties only): slots a * beam + 0 .. rc[a] - 1
    rl, rst, rp  i32 [R]        res_len, res_step, res_par
    seq          2 x i32 [R][P] the hypotheses' tokens, tokens 0 .. t in seq[t & 1] before step t
    step, ctr    i32 [1]

prefilled with sentinels (NaN, ISENT) wherever no token, result or history has been written, so
that "bit-equal to the mirror's state" also says that nothing else was written.

The rule (``mirror_step``), per article that is not done and for t < max_dec:
  candidates (i, j), i < (1 if t == 0 else beam), j < K, in that order, token w = ids[i][j];
  tot = f32(lp[i] + (BLOCKED if ngram_blocked(seq[i], w, n) else lps[i][j]));
  key = tot, or with pen = (inv_len, beta, cpen): f32(f32(tot * inv_len[t + 2]) - f32(beta * cpen[row i]))
  (the product with beta only when cpen is given), the kernel's order of operations;
  walk the candidates by key, descending and stable: a STOP is a result (score key, or
  f32(tot / f32(t + 2)) without penalties; res_lp tot; len t + 2; step t; parent i) from step
  min_dec on and is dropped before; any other token is a new hypothesis (tot, key, w, i); stop at
  beam new hypotheses or beam results in all; done once the article has beam results;
  slot kk < beam takes new hypothesis min(kk, nh - 1); with nh == 0 (-inf, -inf, STOP, parent 0).
A done article, or any at t >= max_dec, gets identity gidx and nothing else."""
import numpy as np

from textsummarization_on_flink_amd.config import HParams
from textsummarization_on_flink_amd.decode.beam_search import inv_len_table, ngram_blocked

f32 = np.float32
BLOCKED = f32(-1e20)
ISENT = -7777
STOP, START = 3, 2
MIN_DEC, MAX_DEC, T_ATT, PITCH = 2, 12, 7, 16
BETA = 0.5
PSTOP = (0.9, 0.6, 0.3, 0.15, 0.05, 0.0)

F_NAMES = ("lp", "key", "rs", "rlp")
I_NAMES = ("latest", "gidx", "th", "ph", "done", "rc", "rl", "rst", "rp", "step", "ctr")
# check name of each state entry (what a failing comparison reports)
CHECK = {"step": "step", "ctr": "ctr", "done": "done", "rc": "res_count", "gidx": "gidx", "th": "tok_hist",
         "ph": "par_hist", "latest": "latest", "lp": "lp_sum", "key": "key_sum", "rl": "res_len", "rst": "res_step",
         "rp": "res_par", "rs": "res_score", "rlp": "res_lp", "seq0": "seq", "seq1": "seq"}


def key_of(tot, il, beta, cp):
    """pen_key (beam_common.h) in its order: two fp32 products, one fp32 difference."""
    key = f32(f32(tot) * f32(il))
    if cp is not None:
        key = f32(key - f32(f32(beta) * f32(cp)))
    return key


def new_state(Na, beam, max_dec=MAX_DEC, P=PITCH):
    R = Na * beam
    st = {"lp": np.zeros(R, f32), "key": np.full(R, np.nan, f32), "rs": np.full(R, np.nan, f32),
          "rlp": np.full(R, np.nan, f32), "latest": np.full(R, ISENT, np.int32), "gidx": np.full(R, ISENT, np.int32),
          "th": np.full((max_dec, R), ISENT, np.int32), "ph": np.full((max_dec, R), ISENT, np.int32),
          "done": np.zeros(Na, np.int32), "rc": np.zeros(Na, np.int32), "rl": np.full(R, ISENT, np.int32),
          "rst": np.full(R, ISENT, np.int32), "rp": np.full(R, ISENT, np.int32), "step": np.zeros(1, np.int32),
          "ctr": np.zeros(1, np.int32), "seq0": np.full((R, P), ISENT, np.int32),
          "seq1": np.full((R, P), ISENT, np.int32)}
    st["seq0"][:, 0] = START
    return st


def copy_state(st):
    return {k: v.copy() for k, v in st.items()}


def mirror_step(st, ids, lps, t, beam, K, stop, min_dec, max_dec, n=0, pen=None):
    """One step on ``st`` (see the module docstring).  Returns the branch counters: blocked
    candidates, articles with equal keys among the reached candidates, results taken, fallback
    slots (kk >= nh > 0), articles with nh == 0; tied_any: articles where a reached candidate's key
    equals that of any other candidate, reached or not."""
    cnt = dict(blocked=0, tied=0, tied_any=0, results=0, fallback=0, nh0=0)
    Na = len(st["done"])
    src, dst = st["seq%d" % (t & 1)], st["seq%d" % ((t + 1) & 1)]
    with np.errstate(all="ignore"):
        for a in range(Na):
            base = a * beam
            if st["done"][a] or t >= max_dec:
                st["gidx"][base:base + beam] = np.arange(base, base + beam)
                continue
            cands = []
            for i in range(1 if t == 0 else beam):
                toks = src[base + i, :t + 1].tolist() if n > 1 else ()
                for j in range(K):
                    w = int(ids[base + i, j])
                    blk = n > 1 and ngram_blocked(toks, w, n)
                    cnt["blocked"] += blk
                    tot = f32(st["lp"][base + i] + (BLOCKED if blk else f32(lps[base + i, j])))
                    key = key_of(tot, pen[0][t + 2], pen[1], None if pen[2] is None else pen[2][base + i]) if pen else tot
                    cands.append((key, tot, i, w))
            order = sorted(range(len(cands)), key=lambda c: cands[c][0], reverse=True)  # stable
            nres, new, seen = int(st["rc"][a]), [], []
            for c in order:
                key, tot, i, w = cands[c]
                seen.append(float(key))
                if w == stop:
                    if t >= min_dec:
                        slot = base + nres
                        st["rs"][slot] = key if pen else f32(tot / f32(t + 2))
                        if pen:
                            st["rlp"][slot] = tot
                        st["rl"][slot], st["rst"][slot], st["rp"][slot] = t + 2, t, i
                        nres += 1
                        cnt["results"] += 1
                else:
                    new.append((tot, key, w, i))
                if len(new) == beam or nres == beam:
                    break
            cnt["tied"] += len(set(seen)) < len(seen)
            allk = [float(c[0]) for c in cands]
            cnt["tied_any"] += any(allk.count(v) > 1 for v in seen)
            st["rc"][a] = nres
            if nres >= beam:
                st["done"][a] = 1
            cnt["nh0"] += not new
            for kk in range(beam):
                cnt["fallback"] += bool(new) and kk >= len(new)
                tot, key, w, i = new[min(kk, len(new) - 1)] if new else (f32(-np.inf), f32(-np.inf), stop, 0)
                r = base + kk
                st["lp"][r], st["latest"][r], st["gidx"][r] = tot, w, base + i
                if pen:
                    st["key"][r] = key
                st["th"][t, r], st["ph"][t, r] = w, i
                if n > 1:
                    dst[r, :t + 1] = src[base + i, :t + 1]
                    dst[r, t + 1] = w
    return cnt


# ------------------------------------------------------------------ named checks
def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def failed_checks(got, exp, names):
    """names of the checks (CHECK) on which ``got`` differs from ``exp`` bit for bit, with the first position"""
    out = {}
    for nm in names:
        g, e = _bits(got[nm]), _bits(exp[nm])
        if g.shape != e.shape or not np.array_equal(g, e):
            bad = np.argwhere(g != e)[0].tolist() if g.shape == e.shape else "shape"
            out.setdefault(CHECK[nm], "%s%s: got %r, mirror %r" % (nm, bad, got[nm][tuple(bad)] if bad != "shape" else g.shape,
                                                                   exp[nm][tuple(bad)] if bad != "shape" else e.shape))
    return out


def state_names(n, pen, ctr):
    names = ["step", "done", "rc", "gidx", "th", "ph", "latest", "lp", "rl", "rst", "rp", "rs"]
    if pen:
        names += ["key", "rlp"]
    if n > 1:
        names += ["seq0", "seq1"]
    if ctr:
        names += ["ctr"]
    return names


def assert_state(tag, got, exp, names):
    bad = failed_checks(got, exp, names)
    assert not bad, "%s: %s" % (tag, "; ".join("[%s] %s" % kv for kv in sorted(bad.items())))


# ------------------------------------------------------------------ the drives of test_gpu_beam_ops 2b
SHAPES = [(1, 2), (2, 4), (3, 6), (5, 10), (4, 8), (8, 8), (16, 4), (1, 1)]
NAS = [1, 6, 70]
MODES = ["plain", "dyadic", "ng2", "ng3", "pen", "ng_pen"]
# seeds chosen (tools of this file: find_seed) so that the conditions of check_conditions hold
SEEDS = {(1, 2, 1, "dyadic"): 5, (2, 4, 1, "dyadic"): 4, (2, 4, 6, "ng3"): 2, (2, 4, 6, "pen"): 3, (2, 4, 6, "ng_pen"): 2,
         (5, 10, 6, "ng_pen"): 1, (4, 8, 6, "ng_pen"): 1, (1, 1, 1, "dyadic"): 1}


def mode_opts(mode):
    """(n, penalties on)"""
    return (2 if mode == "ng2" else 3 if "ng" in mode else 0), "pen" in mode


class Drive:
    """The inputs of MAX_DEC steps from t = 0 plus one call at t = MAX_DEC, and the mirror's state
    after every one of them.

    Candidates: K ids per row out of 40 ordinary ids in a noisy preference order (the beams revisit
    a few tokens, so n-grams repeat); article a's rows carry a [STOP] among their three best with
    probability PSTOP[a % 6] (a single article: 0.15), before and after min_dec = 2: the first
    articles finish mid-run, the last never.  Log-probs: descending multiples of 2^-10 per row,
    distinct ("dyadic": multiples of 1/4 up to min(12, K / 2), drawn with repeats, so that totals
    within a hypothesis and of different hypotheses are equal and the stable order decides).  ng: one live row gets K candidates that are all blocked (step >= 5, as
    soon as a row has a banned token).  pen: wu at alpha 0.9, beta 0.5, cpen multiples of 2^-6."""

    def __init__(self, beam, K, Na, mode, seed=None):
        self.beam, self.K, self.Na, self.mode = beam, K, Na, mode
        self.n, self.use_pen = mode_opts(mode)
        self.seed = SEEDS.get((beam, K, Na, mode), 0) if seed is None else seed
        rng = np.random.default_rng([self.seed, beam, K, Na, MODES.index(mode)])
        R = Na * beam
        self.inv_len = inv_len_table(HParams(length_penalty="wu", length_alpha=0.9), MAX_DEC + 1)
        pool = 10 + np.arange(40)
        st = new_state(Na, beam)
        self.init = copy_state(st)
        self.steps, self.forced = [], None
        self.cnt = dict(blocked=0, tied=0, tied_any=0, results=0, fallback=0, nh0=0)
        self.mid_done = False
        for t in range(MAX_DEC + 1):
            ids = np.zeros((R, K), np.int32)
            for r in range(R):
                ids[r] = pool[np.argsort(np.arange(40) + rng.normal(0, 1.5, 40))][:K]
                if rng.random() < (0.15 if Na == 1 else PSTOP[(r // beam) % 6]):
                    ids[r, rng.integers(0, min(3, K))] = STOP
            dy = mode == "dyadic"
            hi, div = (min(48, 2 * K) + 1, 4) if dy else (3000, 1024)
            lps = -np.sort(np.stack([rng.choice(np.arange(1, hi), K, replace=dy) for _ in range(R)]), 1).astype(f32) / div
            cpen = (rng.integers(0, 256, R) / 64.0).astype(f32)
            att, pg = rng.random((R, T_ATT)).astype(f32), rng.random(R).astype(f32)
            if self.n > 1 and self.forced is None and 5 <= t < MAX_DEC:
                src = st["seq%d" % (t & 1)]
                for r in range(R):
                    if st["done"][r // beam]:
                        continue
                    toks = src[r, :t + 1].tolist()
                    banned = sorted({int(w) for w in pool if ngram_blocked(toks, int(w), self.n)})
                    if banned:
                        ids[r] = [banned[j % len(banned)] for j in range(K)]
                        self.forced = (t, r)
                        break
            c = mirror_step(st, ids, lps, t, beam, K, STOP, MIN_DEC, MAX_DEC, self.n, self.pen(cpen))
            st["step"][0] = t + 1
            for k in c:
                self.cnt[k] += c[k]
            if t == MAX_DEC - 2:
                self.mid_done = bool(st["done"].any())
            self.steps.append(dict(t=t, ids=ids, lps=lps, cpen=cpen, att=att, pg=pg, exp=copy_state(st)))
        self.final = st

    def pen(self, cpen):
        return (self.inv_len, BETA, cpen) if self.use_pen else None

    def names(self, ctr):
        return state_names(self.n, self.use_pen, ctr)

    def conditions(self):
        """what the drive must reach, on the mirror alone: a list of the conditions that fail.  The
        single-article drives and (beam, K) = (1, 1) are exempt from the three conditions on the
        articles' fates: one article cannot both finish and stay live, and at (1, 1) an article
        that meets a lone STOP early goes on with -inf totals.  At beam 1, (1, 2) included, an
        article has 0 or beam results, never something between: that condition needs beam > 1."""
        bad = []
        st, beam = self.final, self.beam
        if self.Na > 1 and (beam, self.K) != (1, 1):
            if not self.mid_done:
                bad.append("no article finished mid-run")
            if st["done"].all():
                bad.append("no article stayed live")
            if beam > 1 and not ((st["rc"] > 0) & (st["rc"] < beam)).any():
                bad.append("no article with 0 < results < beam")
        # (K = 1: one candidate, nothing to tie; beam 1: the walk ends at the first candidate it
        # keeps, so the tie that decides is the one with the candidate behind it)
        if self.mode == "dyadic" and self.K > 1 and self.cnt["tied" if beam > 1 else "tied_any"] < 5:
            bad.append("fewer than 5 tied articles")
        if self.n > 1 and (self.forced is None or self.cnt["blocked"] < self.K):
            bad.append("no forced all-blocked row or fewer than K blocked candidates")
        if (beam, self.K) == (16, 4) and self.cnt["fallback"] < 1:
            bad.append("no fallback slot")
        if (beam, self.K) == (1, 1) and self.cnt["nh0"] < 1:
            bad.append("no nh == 0 step")
        return bad


def find_seed(beam, K, Na, mode, limit=400):
    for seed in range(limit):
        if not Drive(beam, K, Na, mode, seed).conditions():
            return seed
    raise AssertionError("no seed below %d for %r" % (limit, (beam, K, Na, mode)))


# ------------------------------------------------------------------ the mid-run single-step case
MID = dict(beam=16, K=4, Na=3, max_dec=255, P=256, t=250, min_dec=2)


class MidRun:
    """One step entered at t = 250 of max_dec = 255 with P = 256 (beam * P = NG_BAN_MAX) at beam 16,
    K 4: sequences, lp_sum, the result counts (0, 14, 3) and the step counter are prefilled.  Rows
    0 and 1 of article 0 decide a block at the two ends of the ban scan (n = 3): row 0's tokens
    0, 1 equal its last two and token 2 is a candidate (the first int4); row 1's last three tokens
    are equal and that token is a candidate (position t, the last int4)."""

    def __init__(self, form):
        m = MID
        self.form = form
        self.n, self.use_pen = {"plain": (0, False), "ng": (3, False), "pen": (3, True)}[form]
        beam, K, Na, t, P = m["beam"], m["K"], m["Na"], m["t"], m["P"]
        self.beam, self.K, self.Na, self.t = beam, K, Na, t
        R = Na * beam
        rng = np.random.default_rng(250)
        st = new_state(Na, beam, m["max_dec"], P)
        st["seq%d" % (t & 1)][:, :t + 1] = rng.integers(100, 4000, (R, t + 1))  # hardly any n-gram twice
        st["seq%d" % (t & 1)][:, 0] = START
        s = st["seq%d" % (t & 1)]
        s[0, 0:2] = s[0, t - 1:t + 1]
        s[1, t - 2:t + 1] = 77
        st["lp"][:] = -(rng.integers(1 << 10, 1 << 14, R) / 1024.0).astype(f32)
        st["key"][:] = 0
        st["rc"][:] = (0, 14, 3)
        st["step"][0] = t
        self.ids = rng.integers(4, 100, (R, K)).astype(np.int32)
        self.ids[0, 0], self.ids[1, 0] = s[0, 2], 77        # the best candidates of the article's two best rows
        self.ids[[5, 16, 17, 18, 33], 0] = STOP  # article 1 (14 results) meets its STOPs first and finishes
        st["lp"][16:19] = f32(-2.0 ** -10)
        st["lp"][0:2] = f32(-2.0 ** -9), f32(-3 * 2.0 ** -10)
        self.lps = -np.sort(np.stack([rng.choice(np.arange(1, 3000), K, replace=False) for _ in range(R)]), 1) \
            .astype(f32) / 1024
        self.cpen = (rng.integers(0, 256, R) / 64.0).astype(f32)
        self.cpen[16:19] = 0
        self.cpen[0:2] = 0
        self.att, self.pg = rng.random((R, T_ATT)).astype(f32), rng.random(R).astype(f32)
        self.inv_len = inv_len_table(HParams(length_penalty="wu", length_alpha=0.9), m["max_dec"] + 1)
        assert ngram_blocked(s[0, :t + 1].tolist(), int(s[0, 2]), 3) and ngram_blocked(s[1, :t + 1].tolist(), 77, 3)
        assert not ngram_blocked(s[0, 3:t + 1].tolist(), int(s[0, 2]), 3)  # only the match at e = 2 blocks it
        assert not ngram_blocked(s[1, :t].tolist() + [5], 77, 3)           # only position t blocks it
        self.init = copy_state(st)
        self.cnt = mirror_step(st, self.ids, self.lps, t, beam, K, STOP, m["min_dec"], m["max_dec"], self.n,
                               self.pen(self.cpen))
        st["step"][0] = t + 1
        self.exp = st
        if self.n:
            assert self.cnt["blocked"] >= 2
        assert self.cnt["results"] > 0 and st["done"][1] == 1 and st["done"][0] == 0

    def pen(self, cpen):
        return (self.inv_len, BETA, cpen) if self.use_pen else None

    def names(self, ctr):
        return state_names(self.n, self.use_pen, ctr)
