// The acceptance gates of the pipe's follow stage (gr-uwspr_amd/csrc/pipe_rules.h: bytes_rms, follow_gates) on the CPU,
// under ASan + UBSan, against values written down here from the rule as include/uwspr_hip.h states it -- never from the
// code under test.
//   rms:    sqrt(sum_i (byte_i - 128)^2 / 162), the sum in binary32, the root in binary64, rounded to binary32
//   gates:  s_best > 0.12f and rms > (float)(52 * 50 / 64) = 40.625f, both strict; a NaN s_best fails
// usage: follow_rules_main   (from tests/test_follow.py)
#include <math.h>
#include <stdint.h>
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pipe_rules.h"

namespace ru = uwspr::rules;

#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { printf("FAILED %s (line %d)\n", #cond, __LINE__); exit(1); }      \
  } while (0)

static void fill(uint8_t *sym, int lo, int hi) {   // alternating bytes
  for (int i = 0; i < UWSPR_NSYM; i++) sym[i] = (uint8_t)((i & 1) ? hi : lo);
}

static uwspr_follow_result result(float s_best) {
  uwspr_follow_result r;
  memset(&r, 0, sizeof(r));
  r.s_best = s_best;
  return r;
}

int main() {
  uint8_t sym[UWSPR_NSYM];
  fill(sym, 128, 128);
  CHECK(ru::bytes_rms(sym) == 0.0f);
  fill(sym, 128 - 50, 128 + 50);
  CHECK(ru::bytes_rms(sym) == 50.0f);
  fill(sym, 0, 255);                                   // 81 x 128^2 + 81 x 127^2 = 2633553; / 162 = 16256.5; the root 127.5009..
  CHECK(fabsf(ru::bytes_rms(sym) - 127.50098f) < 1e-4f);
  memset(sym, 128, sizeof(sym));
  sym[161] = 0;                                        // one byte: 128^2 / 162 = 101.1358..; the root 10.0566..
  CHECK(fabsf(ru::bytes_rms(sym) - 10.05663f) < 1e-4f);

  fill(sym, 128 - 50, 128 + 50);                       // rms 50 passes; s_best decides, strictly
  CHECK(ru::follow_gates(result(0.45f), sym));
  CHECK(!ru::follow_gates(result(0.12f), sym));
  CHECK(ru::follow_gates(result(nextafterf(0.12f, 1.0f)), sym));
  CHECK(!ru::follow_gates(result(0.0f), sym));
  CHECK(!ru::follow_gates(result(-0.5f), sym));
  CHECK(!ru::follow_gates(result(NAN), sym));
  CHECK(ru::follow_gates(result(INFINITY), sym));

  // the rms gate exactly: 40.625^2 x 162 = 267366.8; 160 bytes at +-40 and two at +-(40 + e) cannot hit it, so take the
  // gate from both sides with whole bytes: all at +-40 (rms 40) fails, all at +-41 (rms 41) passes
  fill(sym, 128 - 40, 128 + 40);
  CHECK(ru::bytes_rms(sym) == 40.0f && !ru::follow_gates(result(0.45f), sym));
  fill(sym, 128 - 41, 128 + 41);
  CHECK(ru::bytes_rms(sym) == 41.0f && ru::follow_gates(result(0.45f), sym));
  // 130 bytes at +-45 and 32 at 128: 130 x 2025 / 162 = 1625; the root 40.311.. fails; 132 at +-45: 1650, 40.62.. fails;
  // 133 at +-45: 1662.5, 40.77.. passes
  for (int n : {130, 132, 133}) {
    memset(sym, 128, sizeof(sym));
    for (int i = 0; i < n; i++) sym[i] = (uint8_t)((i & 1) ? 128 + 45 : 128 - 45);
    CHECK(ru::follow_gates(result(0.45f), sym) == (n == 133));
  }
  memset(sym, 128, sizeof(sym));                       // K16's answer to a NaN or an all-zero frame: no item
  CHECK(!ru::follow_gates(result(0.45f), sym));
  printf("follow rules ok\n");
  return 0;
}
