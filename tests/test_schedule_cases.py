"""The designed frames of tests/schedule_cases.py do on the CPU oracle what they are meant to do: every condition a case
states is asserted here from the oracle alone (no device); the Python replay of the schedule (cc:403-482 over
single-hypothesis calls, the best-of rule written out) equals oracle.demod_candidate on every case, field by field; and
every misreading of the rule the replay can be given changes the expected record of a named case.
tests/test_gpu_schedule_edges.py then holds every form of the schedule to the oracle on the same inputs."""
import numpy as np
import pytest

import schedule_cases as S


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("group", S.GROUPS)
def test_case_conditions_hold_and_replay_is_the_schedule(oracle, group):
    cases = S.group(group)
    assert cases
    for c in cases:
        rec = S.expected(c.name)
        rp, trace = S.traced(c.name)
        assert oracle.record_diff(rp, rec) == [] and S.same_record(rp, rec), (c.name, oracle.record_diff(rp, rec))
        clean = S.expected(c.clean) if c.clean else None
        try:
            c.cond(rec, clean, trace)
        except AssertionError as e:
            raise AssertionError("%s: %s (shift1 %d, sync1 %r, worth %d)" % (c.name, e, rec["shift1"], rec["sync1"], rec["worth_a_try"]))
        print(c.name, rec["shift1"], "%.8f" % rec["sync1"], rec["worth_a_try"],
              "dead tries", [t for t in range(S.NJIG) if rec["worth_a_try"] and S.try_dead(rec, t)])


def test_the_cases_cover_what_they_should():
    names = set(S.CASES)
    a = [c for c in S.group("nonfinite") if c.fkey[0] == "poison" and c.fkey[1] == S.BASE]
    by_sample = {}
    for c in a:
        by_sample.setdefault(c.fkey[2], set()).add(c.fkey[3:])
    assert len(by_sample) == 9 and all(len(v) >= 2 for v in by_sample.values())
    assert len(by_sample[384 + S.W - 1]) == 6 and len(by_sample[320 + S.W - 1]) == 6
    assert set().union(*by_sample.values()) == set(S.VALUES)
    for key in by_sample:                                       # every poisoned frame with all three candidates
        assert sum(1 for c in a if c.fkey[2] == key) == 3 * len(by_sample[key])
    assert {S.MISREADINGS[r] for r in S.MISREADINGS} <= names and set(S.MISREADINGS) == set(S.RULES) - {"reference"}
    assert all(c.clean is None or c.clean in names for c in S.CASES.values())
    for b in (bb for g in S.GROUPS for bb in S.batches(S.group(g))):
        assert sum(len(c) for c in b[1]) <= 42 and len({c.fl for c, _, _ in b[3]}) == 1


def test_a_single_lag_call_is_the_lag_of_a_whole_stage(oracle):
    """the replay's building block: the reference's own five-lag call (mode 0) picks the first maximum of what five
    single-lag calls return, on a frame where the fifth is NaN and on one where all five are bit-equal"""
    for name in ("a_s0_last_nan_i_lin", "c_tie_p8_f2.2"):
        c = S.CASES[name]
        cand = c.cand
        sh = int(cand["shift"])
        sy, lag, f1, _ = oracle.sync_and_demodulate(cand, S.CF, c.frame, float(cand["freq"]), 0, 0, 0.0, sh, sh - 128, sh + 128, 64,
                                                    0.0, 50, 0)
        ms = [S._one(cand, c.frame, cand["freq"], sh + d, 0.0, 0)[0] for d in (-128, -64, 0, 64, 128)]
        with np.errstate(invalid="ignore"):
            q = int(np.nanargmax(ms))
        assert lag == sh + (-128, -64, 0, 64, 128)[q] and np.float32(sy).tobytes() == np.float32(ms[q]).tobytes()
        assert lag == S.traced(name)[1]["lags"]["S1"][0]


@pytest.mark.parametrize("rule", sorted(S.MISREADINGS))
def test_each_misreading_changes_a_named_case(oracle, rule):
    """the proof that the comparisons with the device can fail: a schedule that read the rule this way would return
    another record for the named case (and the replay with the reference rule returns the oracle's)"""
    name = S.MISREADINGS[rule]
    c = S.CASES[name]
    rec = S.expected(name)
    assert S.same_record(S.traced(name)[0], rec)
    wrong = S.replay(c.cand, c.frame, rule=rule)
    diff = oracle.record_diff(wrong, rec)
    print(rule, name, diff, "reference shift1 %d sync1 %r drift1 %r" % (rec["shift1"], rec["sync1"], rec["drift1"]),
          "misread shift1 %d sync1 %r drift1 %r" % (wrong["shift1"], wrong["sync1"], wrong["drift1"]))
    assert diff != [], (rule, name)


def test_misreadings_leave_an_ordinary_frame_alone(oracle):
    """... and none of them shows on the clean base frame: noise plus a signal cannot tell them from the reference"""
    c = S.CASES["a_clean_lin"]
    rec = S.expected("a_clean_lin")
    for rule in sorted(S.MISREADINGS):
        assert S.same_record(S.replay(c.cand, c.frame, rule=rule), rec), rule


# ------------------------------------------------------------------------------------------- e. K1 -> K3 on the scales
def test_front_end_scales_stay_finite_on_the_oracle(oracle):
    """what case (e) rests on: at every scale of E_SCALES the oracle's spectrogram, column averages, smoothed spectrum
    and noise level are finite, one candidate comes back, and it is the unscaled frame's to the byte down to 2^-68
    and not below"""
    fdr = oracle.FDR()
    base = S.frame(S.BASE)
    want = fdr.transform(base)
    assert len(want) == 1
    share = {}
    for k in S.E_SCALES:
        fr = S.frame(("scale", 1.0, k))
        ps = fdr.spectrogram(fr)
        psavg, smraw, smspec, noise = fdr.stats(ps)
        assert np.isfinite(ps).all() and np.isfinite(psavg).all() and np.isfinite(smraw).all()
        assert np.isfinite(smspec).all() and np.isfinite(noise)
        tiny = np.float32(np.finfo(np.float32).tiny)
        share[k] = (float(((ps != 0) & (np.abs(ps) < tiny)).mean()), float((ps == 0).mean()))
        got = fdr.transform(fr)
        assert len(got) == 1, k
        assert (got.tobytes() == want.tobytes()) == (k >= S.E_EQUAL_DOWN_TO), k
    print(share)
    assert share[-60][0] < 1e-3 and share[-60][1] == 0 and share[50] == (0.0, 0.0)
    assert 0 < share[-66][0] < 0.5 < share[-68][0] < share[-72][0] and share[-72][0] > 0.99     # subnormal spectrograms
    assert share[-78][1] > 0.05                                                                  # and exact zeros
