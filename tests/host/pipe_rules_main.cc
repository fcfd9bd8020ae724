// The pure rules of the pipe's fallback path (gr-uwspr_amd/csrc/pipe_rules.h) on the CPU, under ASan + UBSan: the item
// pick, the three acceptance rules and the frequency model, each against a value written down here from the rule as the
// header and include/uwspr_hip.h state it -- never from the code under test.
//   pick:   the try with the largest jig_sync among those with jig_sync > 0.12f and jig_rms > (float)(52 * 50 / 64), both
//           strict, the first one on ties; -1 when none passes (NaN passes no comparison)
//   OSD:    dnext - dmin >= gap, in 64 bits (dnext may be INT32_MAX)
//   list:   0 <= best < M, sbest >= deep_min, and with M > 1 sbest - snext >= deep_gap
//   calls:  0 <= best < 64 * 32400 * 19, sbest >= call_min, and with more than one allowed hypothesis sbest - snext >= call_gap
//   model:  LINEAR (f1, drift1); NONLINEAR (f1 - sgn(V.p) |V.p| / |p| cf / 1500, 0), and (f1, 0) when p = 0
// usage: pipe_rules_main   (from tests/test_host_tail.py)
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pipe_rules.h"

namespace ru = uwspr::rules;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { printf("FAILED %s (line %d)\n", #cond, __LINE__); exit(1); }      \
  } while (0)

static const float kSync = 0.12f, kRms = (float)(52.0 * 50 / 64);   // the gates, as the rule states them

// a record no try of which passes: sync and rms at the gates exactly
static uwspr_demod_out quiet() {
  uwspr_demod_out o;
  memset(&o, 0, sizeof(o));
  for (int t = 0; t < UWSPR_NJIG; t++) { o.jig_sync[t] = kSync; o.jig_rms[t] = kRms; }
  return o;
}
static void gate(uwspr_demod_out &o, int t, float sync) { o.jig_sync[t] = sync; o.jig_rms[t] = 41.0f; }   // 41 > 40.625

static void test_pick() {
  CHECK(kRms == 40.625f);
  uwspr_demod_out o = quiet();
  CHECK(ru::fallback_pick(o) == -1);                       // exactly at both gates: strict, no item
  o.jig_sync[3] = 0.5f;                                    // sync passes, rms at the gate
  CHECK(ru::fallback_pick(o) == -1);
  o.jig_sync[3] = kSync; o.jig_rms[3] = 100.0f;            // rms passes, sync at the gate
  CHECK(ru::fallback_pick(o) == -1);

  o = quiet();                                             // two tries with bit-equal largest sync: the lower index
  gate(o, 11, 0.75f); gate(o, 4, 0.75f); gate(o, 7, 0.5f);
  CHECK(ru::fallback_pick(o) == 4);

  o = quiet();                                             // the largest sync on a try whose rms fails: the next best gated one
  o.jig_sync[2] = 0.9f; o.jig_rms[2] = kRms;
  gate(o, 9, 0.6f); gate(o, 13, 0.3f);
  CHECK(ru::fallback_pick(o) == 9);

  o = quiet();                                             // NaN on every try: no item
  for (int t = 0; t < UWSPR_NJIG; t++) gate(o, t, NAN);
  CHECK(ru::fallback_pick(o) == -1);
  gate(o, 6, 0.2f);                                        // ... and a gated finite one elsewhere: that one
  CHECK(ru::fallback_pick(o) == 6);
  o = quiet();                                             // the NaN first, in front of the finite one
  gate(o, 0, NAN); gate(o, 1, 0.2f);
  CHECK(ru::fallback_pick(o) == 1);

  o = quiet();                                             // only the last try gated
  gate(o, 16, 0.121f);
  CHECK(ru::fallback_pick(o) == 16);
}

static uwspr_osd_result osd(int32_t dmin, int32_t dnext) {
  uwspr_osd_result r;
  memset(&r, 0, sizeof(r));
  r.dmin = dmin; r.dnext = dnext;
  return r;
}

static void test_osd() {
  CHECK(ru::osd_accepts(osd(0, INT32_MAX), 0));            // no runner-up: accepted at any gap, no overflow
  CHECK(ru::osd_accepts(osd(0, INT32_MAX), 485));
  CHECK(ru::osd_accepts(osd(0, INT32_MAX), INT32_MAX));
  CHECK(ru::osd_accepts(osd(40000, INT32_MAX), 485));
  CHECK(ru::osd_accepts(osd(1000, 1485), 485));            // dnext - dmin == gap
  CHECK(!ru::osd_accepts(osd(1000, 1484), 485));           // == gap - 1
  CHECK(ru::osd_accepts(osd(7, 7), 0));
}

static uwspr_deep_result deep(int32_t best, int32_t sbest, int32_t snext) {
  uwspr_deep_result r;
  memset(&r, 0, sizeof(r));
  r.best = best; r.sbest = sbest; r.snext = snext;
  return r;
}

static void test_list() {
  const int smin = 4373, gap = 1145;
  CHECK(ru::list_accepts(deep(0, 4373, 9000), 1, smin, gap));    // M == 1: snext above sbest does not matter
  CHECK(ru::list_accepts(deep(0, 4373, INT32_MIN), 1, smin, gap));
  CHECK(!ru::list_accepts(deep(0, 4372, 0), 1, smin, gap));      // below deep_min
  CHECK(!ru::list_accepts(deep(1, 9000, 0), 1, smin, gap));      // best == M
  CHECK(!ru::list_accepts(deep(2, 9000, 0), 2, smin, gap));
  CHECK(!ru::list_accepts(deep(-1, 9000, 0), 2, smin, gap));     // best == -1
  CHECK(!ru::list_accepts(deep(INT32_MAX, 9000, 0), 2, smin, gap));   // K13's empty winner
  CHECK(ru::list_accepts(deep(1, 6145, 5000), 2, smin, gap));    // M == 2: sbest - snext == gap
  CHECK(!ru::list_accepts(deep(1, 6144, 5000), 2, smin, gap));   // == gap - 1
  CHECK(!ru::list_accepts(deep(0, 4373, 9000), 2, smin, gap));   // what M == 1 took
  CHECK(ru::list_accepts(deep(0, INT32_MAX, INT32_MIN), 2, smin, INT32_MAX));   // 64-bit difference
}

static uwspr_call_result call(int32_t best, int32_t sbest, int32_t snext) {
  uwspr_call_result r;
  memset(&r, 0, sizeof(r));
  r.best = best; r.sbest = sbest; r.snext = snext;
  return r;
}

static void test_calls() {
  const int smin = 5370, gap = 725;
  const int32_t H = 64 * 32400 * 19;                             // hypotheses a result can name
  CHECK(H == 39398400);
  CHECK(ru::calls_accepts(call(0, 5370, 9000), 1, smin, gap));   // one allowed hypothesis: snext does not matter
  CHECK(ru::calls_accepts(call(H - 1, 5370, INT32_MIN), 1, smin, gap));
  CHECK(!ru::calls_accepts(call(0, 5369, 0), 1, smin, gap));     // below call_min
  CHECK(!ru::calls_accepts(call(H, 9000, 0), 1, smin, gap));     // best one past the last hypothesis
  CHECK(!ru::calls_accepts(call(H, 9000, 0), 2, smin, gap));
  CHECK(!ru::calls_accepts(call(-1, 9000, 0), 2, smin, gap));    // best == -1
  CHECK(ru::calls_accepts(call(5, 6725, 6000), 2, smin, gap));   // two: sbest - snext == gap
  CHECK(!ru::calls_accepts(call(5, 6724, 6000), 2, smin, gap));  // == gap - 1
  CHECK(!ru::calls_accepts(call(0, 5370, 9000), 2, smin, gap));  // what one hypothesis took
  CHECK(ru::calls_accepts(call(0, INT32_MAX, INT32_MIN), 39398400LL, smin, INT32_MAX));
}

static void test_model() {
  uwspr_demod_out o;
  memset(&o, 0, sizeof(o));
  o.f1 = 12.625f; o.drift1 = -1.75f;
  uwspr_candidate cd;
  memset(&cd, 0, sizeof(cd));
  float f = 0.0f, d = 99.0f;

  cd.m_type = UWSPR_LINEAR;
  cd.m_linear.drift = 3.0f;                                // (the coarse drift: not what the fine search ended on)
  ru::fine_model(cd, o, 1500.0f, &f, &d);
  CHECK(f == 12.625f && d == -1.75f);

  cd.m_type = UWSPR_NONLINEAR;
  cd.m_nonlinear.V1 = 3.0; cd.m_nonlinear.V2 = 4.0; cd.m_nonlinear.p1 = 0; cd.m_nonlinear.p2 = 0;
  d = 99.0f;
  ru::fine_model(cd, o, 1500.0f, &f, &d);
  CHECK(f == 12.625f && d == 0.0f);                        // p = 0: f1 + 0, no drift
  CHECK(ru::slm_at_zero(cd, 1500.0f) == 0.0f);

  // V.p = 3 * 1 + 4 * 2 = 11 > 0, |p| = sqrt(5): the source closes in, the constant is negative
  const double cf = 1400.0;
  const float mag = (float)(11.0 / sqrt(5.0) * cf / 1500.0);    // binary64, rounded once
  CHECK(mag > 4.59f && mag < 4.60f);                       // 11 / 2.2360680 * 0.9333333 = 4.5914
  cd.m_nonlinear.p1 = 1; cd.m_nonlinear.p2 = 2;
  CHECK(ru::slm_at_zero(cd, (float)cf) == -mag);
  d = 99.0f;
  ru::fine_model(cd, o, (float)cf, &f, &d);
  CHECK(f == 12.625f + -mag && d == 0.0f);
  // V.p = -11 < 0: the same magnitude, the other sign
  cd.m_nonlinear.p1 = -1; cd.m_nonlinear.p2 = -2;
  CHECK(ru::slm_at_zero(cd, (float)cf) == mag);
  d = 99.0f;
  ru::fine_model(cd, o, (float)cf, &f, &d);
  CHECK(f == 12.625f + mag && d == 0.0f);
}

int main() {
  test_pick();
  test_osd();
  test_list();
  test_calls();
  test_model();
  printf("pipe rules ok\n");
  return 0;
}
