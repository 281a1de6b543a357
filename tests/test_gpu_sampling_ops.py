"""Op-level tests of csrc/kernels/sample.hip with no tolerance on the draw.

1. The exact launches of tests/sampling_exact.py: ``out_pick`` and ``out_tok`` of ``sample_full`` /
   ``sample_topk`` EQUAL ``draw_full`` / ``draw_topk`` (planted ties and their twins, every chunk /
   segment / part boundary, V up to the limit 524288 x T = 2048); ``out_lp`` within the bound of
   test_gpu_sampling.py.  The module asserts the number of exact rows it compared.
2. The scalar load path (V not a multiple of 4) under test_gpu_sampling.py's sandwich, unchanged.
3. The bookkeeping tail of both kernels against the plain Python mirror ``sampling_exact.book_step``,
   every buffer inside a sentinel allocation, bit for bit after every step; one graph replay.

profiles/sampling_op_tests.md has the exactness argument and what each launch reaches."""
import numpy as np
import pytest
import torch

import sampling_exact as X
from sampling_exact import MAX_DEC, MIN_DEC, SEED, STOP
from test_gpu_sampling import (NOBOOK, ULP, _check_full_row, _full_ref, _i64, _outs, _step)
from textsummarization_on_flink_amd.decode.sampling import sample_uniform

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT_F, SENT_I = 12288.0, -7777


def _ops():
    from textsummarization_on_flink_amd.ops import ops
    return ops()


def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


# ------------------------------------------------------------------ 1. exact draws
def _run_full(k, L, dev, streams):
    R = L["R"]
    tok, olp, pick = _outs(R)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    k.sample_full(dev["logits"], dev["bias"], dev["pg"] if L["ptr"] else None, dev["attn"] if L["ptr"] else None,
                  dev["ext"], dev["lens"], _dev(streams, torch.long), _step(L["t"]), _i64(SEED), tok, olp, pick, R,
                  L["V"], L["T"], L["rows"], L["stop"], MIN_DEC, MAX_DEC, *NOBOOK, err)
    assert int(err) == 0
    return tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()


def test_sample_full_equals_host_rule_on_exact_inputs():
    k = _ops()
    rows, bad = 0, []
    for L0 in X.full_launches():
        X.check_full(L0)  # the conditions, on the reference inputs, before the launch
        dev = {x: _dev(L0[x]) for x in ("logits", "bias", "pg", "attn", "ext", "lens")}
        for L in [L0] + X.extra_draws(L0):
            tok, olp, pick = _run_full(k, L, dev, L["streams"])
            for r in range(L["R"]):
                rows += 1
                if pick[r] != L["want_pick"][r] or tok[r] != L["want_tok"][r]:
                    bad.append((L["name"], r, L["streams"][r], int(pick[r]), int(L["want_pick"][r])))
            np.testing.assert_allclose(olp, L["want_lp"], rtol=1e-4, atol=1e-5, err_msg=L["name"])
    assert not bad, bad
    assert rows == X.FULL_ROWS == 392


def test_sample_topk_equals_host_rule_on_exact_inputs():
    k = _ops()
    rows, bad = 0, []
    for L in X.topk_launches():
        want = X.check_topk(L)
        R, K = L["R"], L["K"]
        tok, olp, pick = _outs(R)
        k.sample_topk(_dev(L["ids"]), _dev(L["lp"]), _dev(L["streams"], torch.long), _step(L["t"]), _i64(SEED), tok,
                      olp, pick, R, K, L["k"], L["temp"], STOP, MIN_DEC, MAX_DEC, 8, *NOBOOK)
        tok, olp, pick = tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()
        for r in range(R):
            rows += 1
            if pick[r] != want[r] or tok[r] != L["ids"][r, want[r]]:
                bad.append((L["name"], r, int(pick[r]), int(want[r])))
        assert (olp.view(np.int32) == L["lp"][np.arange(R), pick].view(np.int32)).all()
        assert L["t"] >= MIN_DEC or (tok != STOP).all()
    assert not bad, bad
    assert rows == X.TOPK_ROWS == 468


# ------------------------------------------------------------------ 2. the scalar load path
@pytest.mark.parametrize("pointer", [True, False])
@pytest.mark.parametrize("V", [1, 3, 255, 257, 1001, 3001])
def test_sample_full_scalar_path_sandwich(V, pointer):
    """test_sample_full_sandwich's check (its eps formula, its helpers) at V % 4 != 0: rows after the first
    start off a 16-byte boundary and one lane straddles V."""
    from test_gpu_wide_beam import _topk_inputs
    k = _ops()
    T, Na, n, seed = 96, 3, 2, 0xabcdef0123
    R = Na * n
    logits, bias, pg, lens, ext, attn = _topk_inputs(Na, n, V, T, seed=V + pointer)
    ext[:, 5] = STOP
    ext[:, 15] = STOP
    if V > STOP:
        logits[:, STOP] += 6.0
    pg[1], pg[2] = 0.0, 1.0
    assert V % 4 != 0 and logits[1].data_ptr() % 16 != 0
    edges = 0
    for t in (MIN_DEC - 1, MIN_DEC):
        refs = [_full_ref(logits, bias, pg, attn, ext, lens, r, n, t, pointer) for r in range(R)]
        eps = min((V + T + 1.5 * max(x[3] for x in refs) + 8) * ULP, 0.999e-3)
        for base in (0, 2 ** 32 - 3):
            st = list(range(base, base + R))
            tok, olp, pick = _outs(R)
            k.sample_full(logits, bias, pg if pointer else None, attn if pointer else None, ext, lens,
                          torch.tensor(st, dtype=torch.long, device=DEV), _step(t), _i64(seed), tok, olp, pick, R, V, T,
                          n, STOP, MIN_DEC, MAX_DEC, *NOBOOK, None)
            tok, olp, pick = tok.cpu().numpy(), olp.cpu().numpy(), pick.cpu().numpy()
            for r in range(R):
                u = sample_uniform(seed, st[r], t)
                L = int(lens[r // n]) if pointer else 0
                edges += _check_full_row(refs[r], V, L, t, u, int(pick[r]), int(tok[r]), float(olp[r]), eps)
            if pointer:
                assert pick[1] >= V and pick[2] < V
    print(f"sample_full scalar path V={V} pointer={pointer}: {edges} rows inside a widened edge")


# ------------------------------------------------------------------ 3. the bookkeeping tail
def _sbuf(shape, fill, dtype):
    """a buffer of ``shape`` inside an allocation with 64 sentinels behind it: (allocation, view)"""
    n = int(np.prod(shape))
    full = torch.full((n + 64,), SENT_I if dtype == torch.int32 else SENT_F, dtype=dtype, device=DEV)
    full[:n] = fill
    return full, full[:n].view(*shape)


class Books:
    """The device books laid out as ``sampling_exact.book_state`` lays out the mirror."""
    FILL = dict(tok_hist=SENT_I, lp_hist=SENT_F, lp_sum=0.0, latest=2, slen=0, done=0, att_hist=SENT_F, pg_hist=SENT_F)

    def __init__(self, R, T, max_dec, att, pg):
        shapes = dict(tok_hist=(max_dec, R), lp_hist=(max_dec, R), lp_sum=(R,), latest=(R,), slen=(R,), done=(R,))
        if att:
            shapes["att_hist"] = (max_dec, R, T)
        if pg:
            shapes["pg_hist"] = (max_dec, R)
        ints = ("tok_hist", "latest", "slen", "done")
        self.b = {x: _sbuf(s, self.FILL[x], torch.int32 if x in ints else torch.float32) for x, s in shapes.items()}
        self.att = _sbuf((R, T), 0.0, torch.float32) if att else None
        self.pg = _sbuf((R,), 0.0, torch.float32) if pg else None
        self.out = [_sbuf((R,), SENT_I, torch.int32), _sbuf((R,), SENT_F, torch.float32),
                    _sbuf((R,), SENT_I, torch.int32)]

    def args(self):
        v = {x: y[1] for x, y in self.b.items()}
        return (v["done"], v["tok_hist"], v["lp_hist"], v["lp_sum"], v["latest"], v["slen"],
                self.att[1] if self.att else None, v.get("att_hist"), self.pg[1] if self.pg else None, v.get("pg_hist"))

    def outs(self):
        return [x[1] for x in self.out]

    def check(self, st, where):
        for x, (full, view) in self.b.items():
            got = view.cpu().numpy()
            assert np.array_equal(got.view(np.int32), st[x].view(np.int32)), (where, x)
            assert bool((full[view.numel():] == (SENT_I if full.dtype == torch.int32 else SENT_F)).all()), (where, x)
        for full, view in self.out + [y for y in (self.att, self.pg) if y]:
            assert bool((full[view.numel():] == (SENT_I if full.dtype == torch.int32 else SENT_F)).all()), where


R_B, MAXD_B, K_B, KK_B, V_B = 6, 4, 4, 3, 600


def _book_inputs(T, kernel, seed):
    """Per-step inputs on the host; the rows r < 5 with r % 3 == t - 1 can only draw [STOP] at step t (rows 0 and 3
    end at t = 1, 1 and 4 at t = 2, 2 at t = 3; row 5 never ends)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    steps = []
    for t in range(-1, MAXD_B + 1):
        plant = [r for r in range(R_B - 1) if r % 3 == t - 1]
        att, pg = torch.rand(R_B, T, generator=g), torch.rand(R_B, generator=g)
        if kernel == "topk":
            ids = torch.stack([torch.randperm(40, generator=g)[:K_B] + 10 for _ in range(R_B)]).int()
            lp = -torch.rand(R_B, K_B, generator=g).sort(1).values
            for r in plant:
                ids[r, 1], lp[r, 0], lp[r, 2] = STOP, float("-inf"), float("-inf")
            steps.append(dict(ids=ids, lp=lp, att=att, pg=pg))
        else:
            logits = torch.randn(R_B, V_B, generator=g)
            pgen = torch.rand(R_B, generator=g)
            for r in plant:
                logits[r] = float("-inf")
                logits[r, STOP] = 0.5
                pgen[r] = 1.0
            steps.append(dict(logits=logits, pgen=pgen, attn=att / att.sum(1, keepdim=True), att=att, pg=pg))
    return steps


def _book_call(k, kernel, bk, inp, fixed, step, T):
    if bk.att:
        bk.att[1].copy_(inp["att"])
    if bk.pg:
        bk.pg[1].copy_(inp["pg"])
    if kernel == "topk":
        k.sample_topk(inp["ids"].to(DEV), inp["lp"].to(DEV), fixed["streams"], step, _i64(SEED), *bk.outs(), R_B, K_B,
                      KK_B, 1.0, STOP, 0, MAXD_B, T, *bk.args())
    else:
        k.sample_full(inp["logits"].to(DEV), fixed["bias"], inp["pgen"].to(DEV), inp["attn"].to(DEV), fixed["ext"],
                      fixed["lens"], fixed["streams"], step, _i64(SEED), *bk.outs(), R_B, V_B, T, 2, STOP, 0, MAXD_B,
                      *bk.args(), fixed["err"])


def _book_fixed(T):
    g = torch.Generator(device="cpu").manual_seed(T)
    ext = torch.randint(4, V_B + 20, (R_B // 2, T), generator=g, dtype=torch.int32)
    return dict(streams=torch.arange(R_B, dtype=torch.long, device=DEV) + 2 ** 32 - 3,
                bias=torch.randn(V_B, generator=g).to(DEV),
                ext=ext.to(DEV), lens=torch.tensor([T, max(T - 3, 1), max(T // 2, 1)], dtype=torch.int32, device=DEV),
                err=torch.zeros(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("pg", [True, False])
@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("T", [1, 70, 128])
@pytest.mark.parametrize("kernel", ["topk", "full"])
def test_bookkeeping_tail_equals_mirror(kernel, T, att, pg):
    """step = 0 (t = -1: nothing), t = 0 .. 3, then t = 4 >= max_dec (nothing); min_dec = 0 so that the planted [STOP]
    is drawn.  After every step the whole state equals the mirror advanced from the kernel's own out_tok / out_lp."""
    k = _ops()
    bk = Books(R_B, T, MAXD_B, att, pg)
    st = X.book_state(R_B, T, MAXD_B, att, pg)
    fixed = _book_fixed(T)
    prev = [x.cpu().numpy().copy() for x in bk.outs()]
    for n, inp in enumerate(_book_inputs(T, kernel, seed=T + 7)):
        t = n - 1
        done_before = st["done"].copy()
        _book_call(k, kernel, bk, inp, fixed, torch.tensor([n], dtype=torch.int32, device=DEV), T)
        out = [x.cpu().numpy().copy() for x in bk.outs()]
        idle = np.ones(R_B, bool) if (t < 0 or t >= MAXD_B) else done_before.astype(bool)
        for a, b in zip(out, prev):  # rows done before the step, and the idle steps, keep the previous outputs
            assert np.array_equal(a.view(np.int32)[idle], b.view(np.int32)[idle]), (t, "outs")
        if 0 <= t < MAXD_B:
            assert (out[0][~idle] != SENT_I).all() and (out[2][~idle] >= 0).all()
            for r in [r for r in range(R_B - 1) if r % 3 == t - 1 and not idle[r]]:
                assert out[0][r] == STOP
        X.book_step(st, t, out[0], out[1], inp["att"].numpy(), inp["pg"].numpy(), STOP, MAXD_B)
        bk.check(st, (kernel, t))
        prev = out
    assert int(fixed["err"]) == 0
    assert st["slen"].tolist()[:5] == [2, 3, 4, 2, 3] and st["done"].tolist()[:5] == [1] * 5 and st["slen"][5] == 4


@pytest.mark.parametrize("kernel", ["topk", "full"])
def test_bookkeeping_graph_replay_equals_eager(kernel):
    """two steps on fixed inputs, the counter advanced inside the graph: replayed twice == two eager steps"""
    k = _ops()
    T = 70
    inp = _book_inputs(T, kernel, seed=3)[1]
    fixed = _book_fixed(T)
    dinp = {x: y.to(DEV) for x, y in inp.items()}
    res = []
    for graph in (False, True):
        bk = Books(R_B, T, MAXD_B, True, True)
        step = torch.zeros(1, dtype=torch.int32, device=DEV)

        def run():
            step.add_(1)
            if kernel == "topk":
                k.sample_topk(dinp["ids"], dinp["lp"], fixed["streams"], step, _i64(SEED), *bk.outs(), R_B, K_B, KK_B,
                              1.0, STOP, 0, MAXD_B, T, *bk.args())
            else:
                k.sample_full(dinp["logits"], fixed["bias"], dinp["pgen"], dinp["attn"], fixed["ext"], fixed["lens"],
                              fixed["streams"], step, _i64(SEED), *bk.outs(), R_B, V_B, T, 2, STOP, 0, MAXD_B,
                              *bk.args(), fixed["err"])

        bk.att[1].copy_(dinp["att"])
        bk.pg[1].copy_(dinp["pg"])
        if graph:
            allocs = [x[0] for x in list(bk.b.values()) + bk.out]
            keep = [x.clone() for x in allocs]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                run()  # warm-up outside the capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
            for x, y in zip(allocs, keep):
                x.copy_(y)
            step.zero_()
            g.replay()
            g.replay()
        else:
            run()
            run()
        torch.cuda.synchronize()
        assert int(step) == 2
        res.append([x[0].cpu() for x in list(bk.b.values()) + bk.out])
    for x, y in zip(*res):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(res[0][4][:R_B].min()) == 2  # slen: both steps were recorded
