// pipe_rules.h -- the pure rules of the pipe's fallback path (pipe.hip): which try of a record Fano gave up on becomes an
// item, when a fallback's result makes the record a decoded one, and the frequency model a candidate was correlated with.
// Plain C++ on the ABI's records, nothing of HIP and nothing of the pipe: tests/host/pipe_rules_main.cc checks them on the
// CPU against values worked out by hand, and pipe.hip decides by them and by nothing else.
#pragma once

#include <math.h>

#include "../../include/uwspr_hip.h"

namespace uwspr {
namespace rules {

// The gates of decode_try (host_tail.cpp; cc:470), both strict.
constexpr float kMinSync2 = 0.12f;
constexpr float kMinRms = (float)(52.0 * (50 / 64.0));

// The try of a record that the fallbacks take: the gated one with the largest jig_sync, the first one on ties; -1 when no
// try passes the gates (a NaN passes none).  Whether the record is an item at all -- a valid candidate, worth a try, not
// decoded -- is the caller's to say.
static inline int fallback_pick(const uwspr_demod_out &o) {
  int pick = -1;
  for (int idt = 0; idt < UWSPR_NJIG; idt++)
    if (o.jig_sync[idt] > kMinSync2 && o.jig_rms[idt] > kMinRms && (pick < 0 || o.jig_sync[idt] > o.jig_sync[pick])) pick = idt;
  return pick;
}

// A winner is kept when the runner-up is at least `gap` away.  64-bit differences: K9's dnext can be INT32_MAX.
static inline bool gap_holds(int32_t hi, int32_t lo, int gap) { return (long long)hi - (long long)lo >= (long long)gap; }

// K9: the runner-up's distance is at least osd_gap above the winner's (the caller then asks that the bytes unpack)
static inline bool osd_accepts(const uwspr_osd_result &r, int gap) { return gap_holds(r.dnext, r.dmin, gap); }
// K13: a message of the list, its score at least deep_min, and -- with more than one message -- deep_gap above the next
static inline bool list_accepts(const uwspr_deep_result &r, int M, int smin, int gap) {
  return r.best >= 0 && r.best < M && r.sbest >= smin && (M <= 1 || gap_holds(r.sbest, r.snext, gap));
}
// K14: a hypothesis, its score at least call_min, and -- with more than one allowed hypothesis -- call_gap above the next
static inline bool calls_accepts(const uwspr_call_result &r, long long nhyp, int smin, int gap) {
  return r.best >= 0 && r.best < UWSPR_CALLS_MAX * UWSPR_CALL_NGRID * UWSPR_CALL_NPOW && r.sbest >= smin &&
         (nhyp <= 1 || gap_holds(r.sbest, r.snext, gap));
}

// The rms of 162 soft-symbol bytes about 128 as the fine search forms it before its gate (cc:469-474): binary32 sum of
// squares in ascending order, the root in binary64, rounded to binary32.
static inline float bytes_rms(const uint8_t *sym) {
  float sq = 0.0f;
  for (int i = 0; i < UWSPR_NSYM; i++) { const float y = (float)((double)(float)sym[i] - 128.0); sq += y * y; }
  return (float)sqrt((double)sq / 162.0);
}

// K16: the picked hypothesis' sync metric above the fine search's gate and the bytes' rms above its rms gate, both strict (a
// NaN s_best passes neither); the caller then asks that the bytes go through de-interleave, Fano and uwspr_unpack_message
static inline bool follow_gates(const uwspr_follow_result &r, const uint8_t *sym) {
  return r.s_best > kMinSync2 && bytes_rms(sym) > kMinRms;
}

// slmFrequencyDrift (lib/slm.cc:36-73) at t = 0: the constant the fine search adds to a nonlinear candidate's f0
static inline float slm_at_zero(const uwspr_candidate &c, float cf) {
  const double V1 = c.m_nonlinear.V1, V2 = c.m_nonlinear.V2, q1 = (double)c.m_nonlinear.p1, q2 = (double)c.m_nonlinear.p2;
  const float sign = (float)(((q1 * V1 + q2 * V2) > 0) * 2 - 1);
  const double num = fabs(V1 * q1 + V2 * q2), den = sqrt(q1 * q1 + q2 * q2);
  if (den == 0) return 0.0f;
  return (float)((double)(-sign) * num / den * (double)cf / 1500.0);
}

// The frequency model the fine search itself correlated with: f1 and drift1 for a LINEAR candidate; for a NONLINEAR one
// the constant f1 + slmFrequencyDrift(t = 0) (sync_and_demodulate_impl.cc:170-180 evaluates it at t = 0 for every symbol),
// without drift.
static inline void fine_model(const uwspr_candidate &cd, const uwspr_demod_out &o, float cf, float *f_hz, float *drift_hz) {
  if (cd.m_type == UWSPR_NONLINEAR) { *f_hz = o.f1 + slm_at_zero(cd, cf); *drift_hz = 0.0f; }
  else { *f_hz = o.f1; *drift_hz = o.drift1; }
}

}  // namespace rules
}  // namespace uwspr
