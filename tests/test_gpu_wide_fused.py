"""The fused vocab head at beam sizes 6 to 16 (``K = 2 * beam`` up to 32): ``vocab_topk`` /
``vocab_topk_pg`` with the select kernel's 32-entry lists against ``final_topk_wide`` over the very
logits the fused op stored, the refusals that stay, the decoder's choice of step, whole decodes at
beams 8 and 10, and one decode step from a shared state on both heads."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -12345  # id sentinel: no kernel writes it


# ------------------------------------------------------------------ 1. the op against final_topk_wide
def _guarded(rows, cols, dtype, fill):
    """A [rows][cols] buffer between two guard rows (the view the op gets, and the whole)."""
    whole = torch.full((rows + 2, cols), fill, dtype=dtype, device=DEV)
    return whole[1:rows + 1], whole


def _guards_intact(whole, fill):
    for g in (whole[0], whole[-1]):
        ok = torch.isnan(g).all() if fill != fill else (g == fill).all()
        assert bool(ok), "a guard row was written"


def _op_inputs(Na, beam, V, H, T, bias_kind):
    torch.manual_seed(5)
    R = Na * beam
    X = torch.randn(R, H, device=DEV).bfloat16()
    W = (torch.randn(H, V, device=DEV) * 0.3).bfloat16()
    bias = torch.randn(V, device=DEV)
    if bias_kind == "zipf":
        W = (W.float() * 0.05).bfloat16()
        bias = -1.5 * torch.log1p(torch.arange(V, device=DEV, dtype=torch.float32)) + 0.05 * bias
    elif bias_kind == "flat":
        W = torch.zeros_like(W)
        bias = torch.full((V,), 0.25, device=DEV)
    lens = torch.randint(20, T + 1, (Na,), device=DEV, dtype=torch.int32)
    ext = torch.randint(0, V + 20, (Na, T), device=DEV, dtype=torch.int32)
    ext[:, :10] = ext[:, 10:20]  # duplicates
    attn = torch.rand(R, T, device=DEV)
    attn = attn * (torch.arange(T, device=DEV)[None] < lens.repeat_interleave(beam)[:, None]).float()
    attn = attn / attn.sum(1, keepdim=True)
    return X, W.t().contiguous(), bias, lens, ext, attn


def _reference(k, lg, pg, attn, ext, lens, R, V, T, K, beam):
    """final_topk_wide over the logits the fused op stored (bias already in them)."""
    S = int(k.topk_parts(V))
    ids = torch.full((R, K), SENT, dtype=torch.int32, device=DEV)
    lp = torch.full((R, K), float("nan"), device=DEV)
    k.final_topk_wide(lg.contiguous(), torch.zeros(V, device=DEV), pg, attn, ext, lens, ids, lp,
                      torch.zeros(R, S, 2, device=DEV), torch.zeros(R, S, K, device=DEV),
                      torch.zeros(R, S, K, dtype=torch.int32, device=DEV), R, V, T, K, beam)
    return ids, lp


def _check_op(V, H, bias_kind, K, Na=5, beam=None, pg_value=None):
    """One shape at one K in the three forms of the op: p_gen and attention given, neither (the
    baseline model), p_gen computed inside the select.  Returns the pointer form's ids."""
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    beam = K // 2 if beam is None else beam
    T, A, E = 96, 2 * H, 32
    R = Na * beam
    X, WT, bias, lens, ext, attn = _op_inputs(Na, beam, V, H, T, bias_kind)
    pg = torch.rand(R, device=DEV) if pg_value is None else torch.full((R,), pg_value, device=DEV)
    ctx, c, x = torch.randn(R, A, device=DEV), torch.randn(R, H, device=DEV), torch.randn(R, E, device=DEV)
    h = torch.randn(R, H, device=DEV).bfloat16()
    w = torch.randn(A + 2 * H + E, device=DEV) * 0.05
    b = torch.randn(1, device=DEV)
    nt = int(k.vocab_topk_parts(V, H))
    first = None
    for form in ("pointer", "baseline", "pg_inside"):
        ids, ids_all = _guarded(R, K, torch.int32, SENT)
        lp, lp_all = _guarded(R, K, torch.float32, float("nan"))
        lg, lg_all = _guarded(R, V, torch.float32, float("nan"))
        pms, pms_all = _guarded(R, nt * 2, torch.float32, float("nan"))
        pgo_all = torch.full((R + 2,), float("nan"), device=DEV)
        if form == "pointer":
            k.vocab_topk(X, WT, bias, pg, attn, ext, lens, ids, lp, lg, pms, R, V, H, T, K, beam)
            rpg, rattn = pg, attn
        elif form == "baseline":
            k.vocab_topk(X, WT, bias, None, None, ext, lens, ids, lp, lg, pms, R, V, H, T, K, beam)
            rpg, rattn = None, None
        else:
            k.vocab_topk_pg(X, WT, bias, ctx, c, h, x, w, b, pgo_all[1:R + 1], attn, ext, lens, ids, lp, lg, pms, R, V,
                            H, T, K, beam, A, E)
            rpg, rattn = pgo_all[1:R + 1].contiguous(), attn
            ref_pg = torch.sigmoid(torch.cat([ctx, c, h.float(), x], 1) @ w + b)
            assert (rpg - ref_pg).abs().max().item() < 1e-4  # the bound of test_pgen_matches_fp32
            assert bool(torch.isnan(pgo_all[0])) and bool(torch.isnan(pgo_all[-1]))
        torch.cuda.synchronize()
        for whole, fill in ((ids_all, SENT), (lp_all, float("nan")), (lg_all, float("nan")), (pms_all, float("nan"))):
            _guards_intact(whole, fill)
        assert bool(torch.isfinite(lg).all()) and bool((ids != SENT).all()) and bool(torch.isfinite(lp).all())
        ids0, lp0 = _reference(k, lg, rpg, rattn, ext, lens, R, V, T, K, beam)
        torch.cuda.synchronize()
        bad = (ids0 != ids).any(1).nonzero().flatten().tolist()
        assert not bad, (form, bad, ids0[bad[:2]].tolist(), ids[bad[:2]].tolist(), lp0[bad[:2]].tolist(),
                         lp[bad[:2]].tolist())
        err = (lp0 - lp).abs().max().item()
        print(f"V {V} H {H} {bias_kind} K {K} {form}: ids equal on {R} rows, max |dlp| {err:.2e}")
        assert err < 1e-3
        if form == "baseline" and bias_kind == "flat":
            assert ids[0].tolist() == list(range(K))  # equal logits: by id
        first = ids.clone() if first is None else first
    return first, ext, lens


@pytest.mark.parametrize("K", [12, 20, 32])
@pytest.mark.parametrize("V,H,bias_kind", [
    (600, 64, "rand"),      # tile path, 3 tiles: fewer than K
    (600, 128, "rand"),     # span path, 5 span groups: fewer than K
    (3000, 128, "rand"),
    (3000, 128, "flat"),    # every logit equal: order by id
    (50000, 256, "zipf"),   # the trained-bias shape that needs tau2
])
def test_wide_vocab_topk_matches_final_topk_wide(V, H, bias_kind, K):
    """vocab_topk / vocab_topk_pg at K = 12, 20, 32 (5 articles x K / 2 rows, T = 96, ids up to
    V + 20 with duplicates) == final_topk_wide over the logits the fused op stored, with a zero
    bias: both sides select over bit-identical logits, so the ids are equal on every row and the
    log-probs agree within 1e-3.  Every output sits between guard rows."""
    _check_op(V, H, bias_kind, K)


def test_wide_vocab_topk_hidden_512():
    _check_op(50000, 512, "rand", 20)


@pytest.mark.parametrize("V,H,parts", [(9000, 128, 71), (9000, 64, 36), (66000, 128, 258)])
def test_wide_vocab_topk_capacity_worst_case(V, H, parts):
    """Every logit equal at K = 32: the 32 best spans survive every bound unpruned.  4 rows
    (2 articles x 2 rows: the op takes K and the rows per article separately).
    V = 9000, H = 128: the span kernel cuts 9000 columns into 71 groups of at most 128, so 32 x 128
    = 4096 survivors fill the candidate arrays to the last slot.  H = 64 (tile path, 36 tiles of
    256 columns) and V = 66000 (258 span groups, the first 32 of them 256 columns wide) reach
    32 x 256 = 8192 survivors plus the copied ids, twice the arrays: the register passes."""
    from textsummarization_on_flink_amd.ops import ops
    assert int(ops().vocab_topk_parts(V, H)) == parts
    _check_op(V, H, "flat", 32, Na=2, beam=2)


def test_wide_vocab_topk_copy_dominated():
    """p_gen = 0.05 at K = 32, V = 3000: the copy mass outweighs the vocabulary term, so the
    copied ids (in-article OOV ids >= V among them) fill most of the top-32."""
    V, K = 3000, 32
    ids, ext, lens = _check_op(V, 128, "rand", K, pg_value=0.05)
    beam = K // 2
    copied = 0
    for r in range(ids.shape[0]):
        a = r // beam
        copied += len(set(ids[r].tolist()) & set(ext[a, :int(lens[a])].tolist()))
    print("copied ids among the top-32:", copied, "of", ids.numel())
    assert copied > ids.numel() // 2 and bool((ids >= V).any())


# ------------------------------------------------------------------ 2. refusals
def test_vocab_topk_refuses_k33_and_the_beam_tail_refuses_k12():
    from textsummarization_on_flink_amd.ops import ops
    k = ops()
    V, H, T = 600, 64, 32
    zi = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)  # noqa: E731
    zf = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    X, WT = zf(33, H).bfloat16(), zf(V, H).bfloat16()
    nt = int(k.vocab_topk_parts(V, H))
    with pytest.raises(RuntimeError, match="K <= 32"):
        k.vocab_topk(X, WT, zf(V), None, None, zi(1, T), zi(1), zi(33, 33), zf(33, 33), zf(33, V), zf(33, nt, 2), 33, V,
                     H, T, 33, 33)
    R, K, beam, D = 12, 12, 6, 4
    X = zf(R, H).bfloat16()
    with pytest.raises(RuntimeError, match="vocab_topk_beam"):
        k.vocab_topk_beam(X, WT, zf(V), None, None, None, None, None, None, None, None, zi(2, T), zi(2), zi(R, K),
                          zf(R, K), zf(R, V), zf(R, nt, 2), zf(R), zi(R), zi(R), zi(D, R), zi(D, R), zi(2), zi(2), zf(R),
                          zi(R), zi(R), zi(R), zi(1), zi(2), torch.zeros(R, K, dtype=torch.long, device=DEV), zi(1),
                          None, None, R, V, H, T, K, beam, 2 * H, 32, 3, 1, D)


# ------------------------------------------------------------------ 3. decoder wiring
def _decoder(beam, graph=False, wide_beam=False, **kw):
    from test_gpu_wide_beam import _setup
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    hps, vocab, batch, params = _setup(beam, **kw)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=hps.batch_size, T=hps.max_enc_steps, use_graph=graph,
                          wide_beam=wide_beam)
    return d, hps, vocab, batch, params


@pytest.mark.parametrize("beam", [8, 10])
def test_wide_beams_take_the_fused_head(beam, monkeypatch):
    d = _decoder(beam)[0]
    assert d.wide and d.fused_vocab and not d.fused_step
    assert "vpart_ms" in d.b and d.owT is not None
    d = _decoder(beam, wide_beam=True)[0]
    assert d.wide and not d.fused_vocab and not d.fused_step
    monkeypatch.setenv("TSAMD_FUSED_VOCAB", "0")
    d = _decoder(beam)[0]
    assert d.wide and not d.fused_vocab and not d.fused_step


def test_beam4_keeps_its_step():
    """Beam 4 at the production width (H = 256, A = 512: the row attention, so the fused step
    applies): fused_step as before; at beam 10 on the same shape the fused head without it."""
    from textsummarization_on_flink_amd.config import HParams
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus
    from textsummarization_on_flink_amd.decode.device_beam import DeviceBeamDecoder
    from textsummarization_on_flink_amd.models.params import build_params
    Na, T, V = 8, 64, 2000
    hps = HParams(batch_size=Na, max_enc_steps=T, max_dec_steps=16, min_dec_steps=3, beam_size=4, vocab_size=V,
                  emb_dim=128, hidden_dim=256, coverage=True, pointer_gen=True)
    vocab = SyntheticCorpus(vocab_size=V, raw_vocab=3 * V, seed=5, art_mean=50, art_sd=10, sent_mean=4).vocab(V)
    params = build_params(hps, vocab.size(), device="cuda", seed=4)
    d = DeviceBeamDecoder(hps, vocab, params, n_articles=Na, T=T, use_graph=False)
    assert not d.wide and d.row_attn and d.fused_vocab and d.fused_step
    d = DeviceBeamDecoder(hps.replace(beam_size=10), vocab, params, n_articles=Na, T=T, use_graph=False)
    assert d.wide and d.row_attn and d.fused_vocab and not d.fused_step
    d = _decoder(4)[0]  # the small shape of the decodes below
    assert not d.wide and d.fused_vocab and d.fused_step == d.row_attn
    d = _decoder(4, wide_beam=True)[0]
    assert d.wide and not d.fused_vocab and not d.fused_step


# ------------------------------------------------------------------ 4. whole decodes
HEAVY = {"block_ngram_repeat": 3, "length_penalty": "wu", "coverage_penalty_beta": 0.5}


@functools.lru_cache(maxsize=None)
def _fused_graph(beam):
    d, hps, vocab, batch, params = _decoder(beam, graph=True)
    assert d.wide and d.fused_vocab
    return hps, vocab, batch, params, d.decode(batch)


@functools.lru_cache(maxsize=None)
def _oracle_tokens(beam):
    """Host beam search over the fp32 oracle, one article at a time (computed once per beam)."""
    from textsummarization_on_flink_amd.data.batch import Batch, Example
    from textsummarization_on_flink_amd.decode.beam_search import OracleStepModel, run_beam_search
    from textsummarization_on_flink_amd.models.reference import ReferencePointerGenerator
    hps, vocab, batch, params, _ = _fused_graph(beam)
    flat = params.flat
    W = {n: flat[o:o + c].view(params.view(n).shape) for n, (o, c) in params.offsets.items()}
    model = OracleStepModel(ReferencePointerGenerator(hps, vocab.size()), W, hps, device="cuda")
    hps1 = hps.replace(batch_size=hps.beam_size)
    out = []
    for a in range(hps.batch_size):
        ex = Example(batch.original_articles[a], batch.original_abstracts_sents[a], vocab, hps1)
        b1 = Batch([ex] * hps.beam_size, hps1, vocab, pad_enc_to=hps.max_enc_steps)
        out.append(list(run_beam_search(model, vocab, b1, hps).tokens))
    return out


def _agree6(xs, ys):
    n = 0
    for x, y in zip(xs, ys):
        m = min(len(x), len(y), 6)
        n += list(x[:m]) == list(y[:m])
    return n


@pytest.mark.parametrize("beam", [8, 10])
@pytest.mark.parametrize("opt", ["plain", "heavy"])
def test_fused_wide_graph_equals_eager(opt, beam):
    from test_gpu_wide_beam import _pack
    kw = HEAVY if opt == "heavy" else {}
    out = []
    for graph in (True, False):
        d, hps, vocab, batch, params = _decoder(beam, graph=graph, **kw)
        assert d.wide and d.fused_vocab and (d.ngram, d.pen is not None) == ((3, True) if kw else (0, False))
        out.append(_pack(d.decode(batch)))
    assert len(out[0]) == hps.batch_size and [t for t, _, _ in out[0]] == [t for t, _, _ in out[1]]


@pytest.mark.parametrize("beam", [8, 10])
def test_fused_wide_decode_batches_equal_batch_by_batch(beam):
    from test_gpu_wide_beam import _pack
    from textsummarization_on_flink_amd.data.synthetic import SyntheticCorpus, make_batches
    d, hps, vocab, batch, params = _decoder(beam, graph=True)
    corpus = SyntheticCorpus(vocab_size=hps.vocab_size, raw_vocab=3 * hps.vocab_size, seed=9, art_mean=40, art_sd=10,
                             sent_mean=4)
    batches = [batch] + make_batches(hps, vocab, corpus, 2, pad_enc_to=hps.max_enc_steps)
    assert d.fused_vocab and d.group_enc > 1
    seq = [_pack(d.decode(b)) for b in batches]
    assert [_pack(hy) for hy in d.decode_batches(batches)] == seq


@pytest.mark.parametrize("beam", [8, 10])
def test_fused_wide_tracks_materialised_decoder_and_host_oracle(beam):
    """The first 6 tokens of the fused decoder agree with the ``wide_beam=True`` decoder
    (materialised logits: the two differ only in the logits' summation order) and with the host
    search over the fp32 oracle on at least Na - 2 articles each, the criterion of
    test_wide_beam_tracks_host_oracle."""
    hps, vocab, batch, params, hf = _fused_graph(beam)
    m = _decoder(beam, graph=True, wide_beam=True)[0]
    assert not m.fused_vocab
    hm = m.decode(batch)
    ft, mt, ot = [h.tokens for h in hf], [h.tokens for h in hm], _oracle_tokens(beam)
    Na = hps.batch_size
    a_fm, a_fo, a_mo = _agree6(ft, mt), _agree6(ft, ot), _agree6(mt, ot)
    print(f"beam {beam}: first 6 tokens agree on fused/materialised {a_fm}, fused/oracle {a_fo}, "
          f"materialised/oracle {a_mo} of {Na}")
    assert a_fm >= Na - 2 and a_fo >= Na - 2, (a_fm, a_fo, a_mo)


# ------------------------------------------------------------------ 5. one step from the same state
def test_one_step_same_state_both_heads():
    """The state of a fused beam-10 decoder after its prologue, copied into a ``wide_beam=True``
    decoder; one ``_step`` on each.  top_ids agree as sets on every row, except rows whose
    materialised log-probs at rank K and rank K + 1 are closer than 1e-3 (there the logits'
    summation order may decide); at most 1 row in 10 may be so excused."""
    f, hps, vocab, batch, params = _decoder(10)
    m = _decoder(10, wide_beam=True)[0]
    assert f.fused_vocab and not m.fused_vocab
    f._encode(batch)
    f._prologue()
    m._encode(batch)
    m._prologue()
    for name, t in f.b.items():
        if name in m.b and m.b[name].shape == t.shape:
            m.b[name].copy_(t)
    for sf, sm in zip(f.st, m.st):
        for name in sf:
            sm[name].copy_(sf[name])
    f._step(0)
    m._step(0)
    torch.cuda.synchronize()
    R, K, V, T, beam = f.R, f.K, f.V, f.T, f.beam
    # the materialised side's whole extended distribution, for the gap at the cut
    from textsummarization_on_flink_amd.models.pointer_generator import OV
    pg = m.b["PG"].double()[:, None]
    vd = torch.softmax(m.b["logits"].double() + params[OV].double(), 1)
    fd = torch.cat([pg * vd, torch.zeros(R, T, device=DEV, dtype=torch.float64)], 1)
    att = m.st[1]["ATT"].double()
    att = att * (torch.arange(T, device=DEV)[None] < m.b["lens"].repeat_interleave(beam)[:, None])
    fd = fd.scatter_add(1, m.b["ext"].repeat_interleave(beam, 0).long(), (1 - pg) * att)
    top = torch.sort(fd, 1, descending=True).values[:, :K + 1].log()
    tie = ((top[:, K - 1] - top[:, K]) < 1e-3).tolist()
    fi, mi = f.b["top_ids"].tolist(), m.b["top_ids"].tolist()
    differ = [r for r in range(R) if set(fi[r]) != set(mi[r])]
    excused = [r for r in differ if tie[r]]
    print(f"one step, beam 10: {R} rows, {len(differ)} differ, {len(excused)} of them excused; rows with a "
          f"gap under 1e-3 at the cut: {sum(tie)}")
    assert all(tie[r] for r in differ), [r for r in differ if not tie[r]]
    assert len(excused) * 10 <= R
    assert (f.b["PG"] - m.b["PG"]).abs().max().item() < 1e-4
