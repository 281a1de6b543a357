"""CPU tier of tests/test_gpu_beam_ops.py: the drives reach what they claim (conditions asserted on
the mirror alone), a numpy emulation of the kernel's PARALLEL form (beam_step_body: rank by
counting, exclusive ballot / popcount positions, ``reached = nn < beam && nres0 + ns < beam``, slot
fill; the int4 ban scan) passes every drive against the sequential mirror, and each planted mistake
in that emulation is rejected by a named check (profiles/beam_op_tests.md holds the table)."""
import numpy as np
import pytest

import beam_mirror as M
from beam_mirror import BLOCKED, MAX_DEC, MIN_DEC, STOP, f32

MUTATIONS = {
    # name: the checks of which at least one must reject it
    "tie_high": {"tok_hist", "par_hist"},        # ties broken towards the higher candidate index
    "inclusive": {"res_count", "tok_hist"},      # inclusive instead of exclusive counts
    "no_nres0": {"res_count", "done"},           # nres0 ignored in ``reached``
    "t0_all_rows": {"tok_hist", "par_hist"},     # all beam rows used at t == 0
    "parent_mod": {"par_hist", "gidx"},          # parent taken as lane % K
    "early_stop": {"res_count"},                 # STOP before min_dec counted as a result
    "len_t1": {"res_len"},                       # res_len = t + 1
    "score_t1": {"res_score"},                   # score divided by t + 1
    "drop_blocked": {"tok_hist", "lp_sum"},      # a blocked candidate dropped instead of ranked last
    "suffix_n": {"tok_hist", "lp_sum"},          # suffix match over n tokens instead of n - 1
    "scan_short": {"tok_hist", "lp_sum"},        # ban scan stopping one int4 early
    "inv_len_t1": {"key_sum", "res_score"},      # key from inv_len[t + 1]
    "cpen_child": {"key_sum", "tok_hist"},       # cpen of a child slot instead of the parent row
    "lp_is_key": {"lp_sum"},                     # lp_sum carrying the key
    "fallback_first": {"tok_hist", "lp_sum"},    # fallback slot repeats the first new hypothesis
    "done_no_gidx": {"gidx"},                    # done article not given identity gidx
}


def emu_step(st, ids, lps, t, beam, K, stop, min_dec, max_dec, n=0, pen=None, mut=None):
    """beam_step_kernel with ctr = None on the state of beam_mirror, 64 lanes per article at once."""
    Na = len(st["done"])
    R = Na * beam
    src, dst = st["seq%d" % (t & 1)], st["seq%d" % ((t + 1) & 1)]
    P = src.shape[1]
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for a in range(Na):
            base = a * beam
            if st["done"][a] or t >= max_dec:
                if mut != "done_no_gidx":
                    st["gidx"][base:base + beam] = np.arange(base, base + beam)
                continue
            nres0 = int(st["rc"][a])
            valid = lane < beam * K
            li, lj = np.where(valid, lane // K, 0), np.where(valid, lane % K, 0)
            lp_row = st["lp"][base + li]
            tot = np.where(valid, (lp_row + lps[base + li, lj]).astype(f32), f32(-np.inf)).astype(f32)
            tid = np.where(valid, ids[base + li, lj], 0)
            dropped = np.zeros(64, bool)
            if n > 1:  # ngram_ban_build + ngram_banned
                t4 = (t + 4) & ~3
                ban = np.full((beam, P), -1, np.int64)
                m = n + 1 if mut == "suffix_n" else n
                for i in range(beam):
                    s = src[base + i]
                    for e in range(t4):
                        if m - 1 <= e <= t and all(s[e - k] == s[t + 1 - k] for k in range(1, m)):
                            ban[i, e] = s[e]
                nq = (t >> 2) + (0 if mut == "scan_short" else 1)
                hit = np.array([valid[l] and tid[l] in ban[li[l], :4 * nq] for l in range(64)])
                if mut == "drop_blocked":
                    dropped = hit
                tot = np.where(hit, (lp_row + BLOCKED).astype(f32), tot).astype(f32)
            norig = beam if (t > 0 or mut == "t0_all_rows") else 1
            ncand = norig * K
            tot = np.where(lane >= ncand, f32(-np.inf), tot).astype(f32)
            key = tot
            if pen:
                il = f32(pen[0][t + 1 if mut == "inv_len_t1" else t + 2])
                key = (tot * il).astype(f32)
                if pen[2] is not None:
                    row = base + (lane % beam if mut == "cpen_child" else li)
                    key = (key - (f32(pen[1]) * pen[2][row]).astype(f32)).astype(f32)
                key = np.where(lane < ncand, key, f32(-np.inf)).astype(f32)
            act0 = (lane < ncand) & ~dropped
            if mut == "drop_blocked":
                key = np.where(dropped, f32(-np.inf), key).astype(f32)
            # stable rank by counting
            q = lane[:ncand]
            tie = (q[None, :] > lane[:, None]) if mut == "tie_high" else (q[None, :] < lane[:, None])
            rank = ((key[None, :ncand] > key[:, None]) | ((key[None, :ncand] == key[:, None]) & tie)).sum(1)
            cval, ckey, cid, srt = np.zeros(64, f32), np.zeros(64, f32), np.zeros(64, np.int64), np.zeros(64, np.int64)
            live = np.zeros(64, bool)
            for l in range(ncand):
                cval[rank[l]], ckey[rank[l]], cid[rank[l]] = tot[l], key[l], tid[l]
                srt[rank[l]] = l % K if mut == "parent_mod" else l // K
                live[rank[l]] = act0[l]
            act = (lane < ncand) & live
            is_res = act & (cid == stop) & ((t >= min_dec) or mut == "early_stop")
            is_hyp = act & (cid != stop)
            ns, nn = np.cumsum(is_res), np.cumsum(is_hyp)
            if mut != "inclusive":
                ns, nn = ns - is_res, nn - is_hyp
            reached = act & (nn < beam) & ((ns if mut == "no_nres0" else nres0 + ns) < beam)
            nlp, nkey = np.zeros(beam + 1, f32), np.zeros(beam + 1, f32)
            ntok, npar = np.zeros(beam + 1, np.int64), np.zeros(beam + 1, np.int64)
            for l in range(64):
                if reached[l] and is_res[l]:
                    slot = base + nres0 + ns[l]
                    if slot >= R:
                        continue
                    if pen:
                        st["rs"][slot], st["rlp"][slot] = ckey[l], cval[l]
                    else:
                        st["rs"][slot] = f32(cval[l] / f32(t + 1 if mut == "score_t1" else t + 2))
                    st["rl"][slot] = t + 1 if mut == "len_t1" else t + 2
                    st["rst"][slot], st["rp"][slot] = t, srt[l]
                if reached[l] and is_hyp[l]:
                    nlp[nn[l]], nkey[nn[l]], ntok[nn[l]], npar[nn[l]] = cval[l], ckey[l], cid[l], srt[l]
            nres = nres0 + int((is_res & reached).sum())
            nh = int((is_hyp & reached).sum())
            st["rc"][a] = nres
            if nres >= beam:
                st["done"][a] = 1
            adv = []
            for k in range(beam):
                kk = k if k < nh else (0 if mut == "fallback_first" else max(nh - 1, 0))
                par = int(npar[kk]) if nh > 0 else 0
                r = base + k
                st["lp"][r] = (nkey[kk] if (mut == "lp_is_key" and pen) else nlp[kk]) if nh > 0 else f32(-np.inf)
                if pen:
                    st["key"][r] = nkey[kk] if nh > 0 else f32(-np.inf)
                tok = int(ntok[kk]) if nh > 0 else stop
                st["latest"][r], st["gidx"][r] = tok, base + par
                st["th"][t, r], st["ph"][t, r] = tok, par
                adv.append((par % beam, tok))
            if n > 1:  # ngram_seq_advance
                for k, (par, tok) in enumerate(adv):
                    dst[base + k, :t + 1] = src[base + par, :t + 1]
                    dst[base + k, t + 1] = tok
    st["step"][0] = t + 1


def _emu_drive(d, mut=None):
    """every step of a drive from the mirror's state before it: the names of the failing checks"""
    bad = {}
    pre = d.init
    for s in d.steps:
        st = M.copy_state(pre)
        emu_step(st, s["ids"], s["lps"], s["t"], d.beam, d.K, STOP, MIN_DEC, MAX_DEC, d.n, d.pen(s["cpen"]), mut)
        for k, v in M.failed_checks(st, s["exp"], d.names(False)).items():
            bad.setdefault(k, "t=%d %s" % (s["t"], v))
        pre = s["exp"]
    return bad


def _emu_mid(m, mut=None):
    st = M.copy_state(m.init)
    st["step"][0] = m.t + 1
    emu_step(st, m.ids, m.lps, m.t, m.beam, m.K, STOP, M.MID["min_dec"], M.MID["max_dec"], m.n, m.pen(m.cpen), mut)
    return M.failed_checks(st, m.exp, m.names(False))


@pytest.mark.parametrize("Na", M.NAS)
@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("beam,K", M.SHAPES)
def test_drive_reaches_its_branches_and_emulation_matches(beam, K, mode, Na):
    d = M.Drive(beam, K, Na, mode)
    assert not d.conditions(), (d.conditions(), d.cnt, d.final["rc"].tolist())
    assert len(d.steps) == MAX_DEC + 1 and d.steps[-1]["exp"]["step"][0] == MAX_DEC + 1
    bad = _emu_drive(d)
    assert not bad, bad


@pytest.mark.parametrize("form", ["plain", "ng", "pen"])
def test_mid_run_case_and_emulation(form):
    m = M.MidRun(form)
    assert M.MID["beam"] * M.MID["P"] == 4096  # NG_BAN_MAX (launchers.h)
    assert not _emu_mid(m)


def _mutation_inputs():
    out = [M.Drive(4, 8, 6, mode) for mode in M.MODES]
    out += [M.Drive(16, 4, 6, "plain"), M.Drive(5, 10, 6, "ng_pen"), M.Drive(1, 1, 6, "plain"), M.Drive(1, 2, 6, "ng2")]
    return out


@pytest.fixture(scope="module")
def mutation_inputs():
    return _mutation_inputs(), [M.MidRun(f) for f in ("plain", "ng", "pen")]


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_planted_mistake_is_rejected(mut, mutation_inputs):
    drives, mids = mutation_inputs
    failed = {}
    for d in drives:
        for k, v in _emu_drive(d, mut).items():
            failed.setdefault(k, "%s %s" % ((d.beam, d.K, d.Na, d.mode), v))
    for m in mids:
        for k, v in _emu_mid(m, mut).items():
            failed.setdefault(k, "mid-run %s %s" % (m.form, v))
    print(mut, "rejected by", sorted(failed))
    assert MUTATIONS[mut] & set(failed), (mut, failed)


def test_scan_short_is_caught_by_the_mid_run_case_alone():
    """the last int4 of the ban scan decides only when position t holds the banned token: the
    mid-run case's row 1"""
    assert _emu_mid(M.MidRun("ng"), "scan_short")
