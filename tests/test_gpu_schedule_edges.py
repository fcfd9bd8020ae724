"""The refinement schedule S0-S5 on DESIGNED frames, in every form the library has, against the CPU oracle: one
non-finite sample in one lag's window and not in its neighbour's, the frame's first and last sample, bit-equal metrics,
subnormal and infinite products.  The inputs and what each of them reaches are in tests/schedule_cases.py; that they
reach it, and that a schedule which misread the best-of rule would return other records for them, is asserted on the
oracle alone in tests/test_schedule_cases.py.  Here every record of every form is held to oracle.demod_candidate with
oracle.record_diff: all fields, the 17 tries' soft symbols, shifts and metrics by bytes.

Several cases travel in one call (schedule_cases.batches), so that poisoned and clean frames, live and dead slots share
workgroups.
"""
import numpy as np
import pytest

import schedule_cases as S

pytestmark = pytest.mark.gpu

# the option sets of test_schedule_forms_are_identical (tests/test_gpu_parity.py)
FORMS = ({"sched": 1},
         {"sched": 0, "stage_kernels": 0, "reuse": 0, "phasor_tables": 0},
         {"sched": 0, "stage_kernels": 0},
         {"sched": 0, "stage_kernels": 1},
         {"sched": 0, "stage_kernels": 1, "reuse": 0},
         {"sched": 0, "stage_kernels": 1, "phasor_tables": 0},
         {"sched": 0, "stage_kernels": 1, "k4_forms": 0},
         {"sched": 0, "stage_kernels": 1, "k4_forms": 0, "reuse": 0},
         {"sched": 1, "reuse": 0})


def make_contexts(G, **kw):
    made = []
    for opts in FORMS:
        c = G.Context(options=opts, **kw)
        assert all(c.get_option(k) == v for k, v in opts.items())
        made.append((opts, c))
    return made


@pytest.fixture(scope="module")
def ctxs(G, oracle):
    """the nine contexts, created once"""
    made = make_contexts(G)
    yield made
    for _, c in made:
        c.close()


def launches(opts, lazy=False):
    """what one demod_batch on hand-made candidates launches through the counted launchers (uwspr_debug_launch_forms):
    the fused kernel goes through none of them; the staged form with the flat kernel sends all six stages through it;
    with the stage kernels the flat kernel takes the drifting candidates' part of S0 and of S2 (and a lazy S5).  At
    these sizes the flat kernel runs with one tone per lane and the fold in its wave form; the last fold carries the
    soft symbols and the winner's magnitudes."""
    if opts["sched"] == 1:
        return {}
    flat = 6 if opts.get("stage_kernels", 1) == 0 else (3 if lazy else 2)
    return {"flat_t1": flat, "fold_wave": 1, "fold_wave_soft": 1, "fold_wave_pwin": 1}


def delta(after, before):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def run_forms(ctxs, cases, oracle):
    """every batch of `cases` through every context; -> the records of the first form, {case name: record}"""
    bad, first = [], {}
    for frames, cands, per, where in S.batches(cases):
        for q, (opts, ctx) in enumerate(ctxs):
            before = ctx.launch_forms()
            out = ctx.demod_batch(frames, cands, max_per_frame=per)
            assert delta(ctx.launch_forms(), before) == launches(opts), opts
            for c, b, j in where:
                d = oracle.record_diff(out[b, j], S.expected(c.name))
                if d:
                    bad.append((c.name, opts, d, int(out[b, j]["shift1"]), float(out[b, j]["sync1"])))
                if q == 0:
                    first[c.name] = out[b, j].copy()
            for b in range(len(cands)):                     # the slots behind a frame's last candidate stay empty
                for j in range(len(cands[b]), per):
                    assert int(out[b, j]["worth_a_try"]) == 0 and not out[b, j]["symbols"].any(), (opts, b, j)
    assert bad == [], "%d records differ from the oracle:\n%s" % (len(bad), "\n".join(map(repr, bad[:40])))
    return first


@pytest.mark.parametrize("group", ["nonfinite", "edges", "ties", "scale"])
def test_designed_frames_in_every_form(ctxs, oracle, group):
    """cases a (one non-finite sample), b (first and last sample), c (exact ties), d (scale): nine forms, each record
    against the oracle"""
    got = run_forms(ctxs, S.group(group), oracle)
    assert set(got) == {c.name for c in S.group(group)}


def test_samples_from_45000_on_in_every_form(G, oracle):
    """case b with fl = 48 000: a NaN at sample 45 000 is never read (np = 45 000, cc:92), one at 44 999 is"""
    made = make_contexts(G, fl=48000)
    try:
        got = run_forms(made, S.group("late48"), oracle)
    finally:
        for _, c in made:
            c.close()
    assert got["b_late48_nan45000"].tobytes() == got["b_late48_clean"].tobytes()
    assert got["b_late48_nan44999"].tobytes() != got["b_late48_clean"].tobytes()


@pytest.mark.parametrize("form", [0, 3], ids=["fused", "staged"])
def test_lazy_tries_and_resume_on_designed_frames(ctxs, oracle, form):
    """cases a and c lazily (uwspr_set_tries 1 and 3), then resumed: the stage results and the wanted tries are the
    eager ones, the rest is zero; after the resume the flagged records equal the eager records byte for byte -- dead
    tries, tied tries and the reuse of try 0 included -- and the unflagged ones are untouched.  Both schedule forms, as
    test_lazy_tries_and_resume_equal_the_eager_schedule."""
    opts, ctx = ctxs[form]
    for frames, cands, per, where in S.batches(S.group("nonfinite") + S.group("ties")):
        eager = ctx.demod_batch(frames, cands, max_per_frame=per)
        for c, b, j in where:
            assert oracle.record_diff(eager[b, j], S.expected(c.name)) == [], (c.name, opts)
        try:
            for k in (1, 3):
                ctx.set_tries(k)
                before = ctx.launch_forms()
                lazy = ctx.demod_batch(frames, cands, max_per_frame=per)
                assert delta(ctx.launch_forms(), before) == launches(opts, lazy=True), (opts, k)
                for f in ("f1", "drift1", "sync1", "shift1", "worth_a_try"):
                    assert lazy[f].tobytes() == eager[f].tobytes(), (k, f)
                for f in ("symbols", "jig_sync", "jig_rms"):
                    assert lazy[f][:, :, :k].tobytes() == eager[f][:, :, :k].tobytes(), (k, f)
                assert not lazy["symbols"][:, :, k:].any() and not lazy["jig_sync"][:, :, k:].any()
                need = np.zeros((len(cands), per), np.uint8)
                need[0::2, :] = 1
                need[1::2, 0] = 1
                res = ctx.demod_resume(frames, need, None, max_per_frame=per)
                for b in range(len(cands)):
                    for j in range(per):
                        want = eager[b, j] if need[b, j] else lazy[b, j]
                        assert res[b, j].tobytes() == want.tobytes(), (opts, k, b, j)
        finally:
            ctx.set_tries(17)


@pytest.mark.parametrize("sched", [1, 0], ids=["fused", "staged"])
def test_front_end_and_pipeline_on_scaled_frames(G, oracle, sched):
    """case e: K1 -> K3 and the schedule behind them (uwspr_pipeline_batch: the S0 lag-group launch of the staged form
    is left out) on frames scaled by 2^k, where the spectrogram is subnormal in part (-66), mostly (-68), wholly (-72)
    or holds exact zeros (-78): spectrogram band, statistics, candidates and records against the oracle, by bytes"""
    frames = np.stack([S.frame(S.BASE)] + [S.frame(("scale", 1.0, k)) for k in S.E_SCALES])
    fdr = oracle.FDR()
    ctx = G.Context(options={"sched": sched})
    try:
        got = ctx.fdr_batch(frames)
        ps, psavg, smraw, smspec, noise = ctx.fdr_spectrum(len(frames))
        before = ctx.launch_forms()
        cands, out = ctx.pipeline_batch(frames, max_per_frame=2)
        forms = delta(ctx.launch_forms(), before)
        lo, w = ctx.info.band_lo, ctx.info.band_w
    finally:
        ctx.close()
    assert forms == ({} if sched else {"fold_wave": 1, "fold_wave_soft": 1, "fold_wave_pwin": 1})   # no flat launch at all
    bad = []
    for b, k in enumerate((0,) + S.E_SCALES):
        ops = fdr.spectrogram(frames[b])
        opsavg, osmraw, osmspec, onoise = fdr.stats(ops)
        exp = fdr.transform(frames[b])
        assert len(exp) == 1
        for name, a, e in (("ps", ps[b], ops[:, lo:lo + w]), ("psavg", psavg[b], opsavg[lo:lo + w]), ("smraw", smraw[b], osmraw),
                           ("smspec", smspec[b], osmspec), ("noise", noise[b], np.float32(onoise))):
            if np.ascontiguousarray(a).tobytes() != np.ascontiguousarray(e).tobytes():
                bad.append((k, name, int((np.asarray(a) != np.asarray(e)).sum())))
        for tag, lst in (("fdr_batch", got[b]), ("pipeline_batch", cands[b])):
            if len(lst) != len(exp):
                bad.append((k, tag, "%d candidates, the oracle %d" % (len(lst), len(exp))))
            else:
                bad += [(k, tag, oracle.cand_diff(a, e)) for a, e in zip(lst, exp) if oracle.cand_diff(a, e)]
        d = oracle.record_diff(out[b, 0], oracle.demod_candidate(exp[0], S.CF, frames[b]))
        if d:
            bad.append((k, "record", d))
        assert int(out[b, 1]["worth_a_try"]) == 0 and not out[b, 1]["symbols"].any()
    assert bad == [], bad
