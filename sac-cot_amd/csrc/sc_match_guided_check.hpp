// sc_match_guided_check.hpp — the host-only rules of sc_match_guided (include/saccot.h): what is refused of sc_guide_params, and how
// the threshold of the gate is derived.  No HIP: sc_capi_match.hip includes it, and so does tests/native/match_guided_check_main.cpp,
// a program of its own that runs these functions under the sanitizers on the CPU.
#pragma once
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/saccot.h"

namespace sc {

// What a call refuses of its guide block — the rule that is broken, for the caller to put its name in front of; nullptr: it is fine.
// The gate: finite and > 0, so the smallest subnormal and FLT_MAX are both accepted (the first admits nothing: its square is 0;
// the second squares to +inf, which still admits no infinite residual: inf < inf is false).
inline const char* guide_params_error(const sc_guide_params* gp) {
  if (gp->size != sizeof(sc_guide_params)) return "guide->size is not sizeof(sc_guide_params)";
  if (gp->layout > (uint32_t)SC_SOA) return "guide->layout must be SC_AOS or SC_SOA";
  if (!(gp->gate > 0.f && gp->gate <= FLT_MAX)) return "guide->gate must be finite and > 0";
  if (gp->flags != 0) return "guide->flags must be 0";
  if (gp->reserved[0] || gp->reserved[1] || gp->reserved[2] || gp->reserved[3]) return "a reserved field of guide is not 0";
  return nullptr;
}

// gate^2 as tau^2 is derived: the fp32 parameter squared in fp64, rounded once
inline float guide_gate2(float gate) { return (float)((double)gate * (double)gate); }

}  // namespace sc
