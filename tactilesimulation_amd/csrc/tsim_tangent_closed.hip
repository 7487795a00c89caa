// tsim_tangent_closed.hip — the forward-mode tangent pass through the fused closed-loop episode (include/tsim_env.h tsim_push_closed_tangent; the math:
// there and DESIGN.md §4 "Closed-loop tangent pass").
//   k_closed_tangent   k_tangent's body (tsim_tangent_kernel.h ts_tangent_walk) with POLICY on: the sub-step code is k_tangent's, instruction for
//                      instruction in the source; at a frame's start the frame's du comes from the policy's tangent evaluated in the slot
//                      (tsim_tangent_closed.h), whose tactile input is the tactile tangent this slot wrote at the previous frame's end.  SRC = true adds
//                      the body columns' source (k_tangent_body_src ran first, unchanged: its source depends on the taped state only).
// TactilePush only (7 dofs: NRM 8, no rotation-vector joint), generic view only, 16 / 32 / 64 lanes as k_tangent's plan chooses them.
// It reads the tape, the policy's weights and forward records, and writes the caller's buffers, nothing else.
// Built like the generic kernels (tsim_hip.hip): no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_tangent.h"
#include "tsim_tangent_closed.h"
#include "tsim_tangent_kernel.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE, bool SRC>
__global__ void __launch_bounds__(TS_WAVE) k_closed_tangent(TanClosedArgs<R> a) { ts_tangent_walk<R, NRM, EXPJ, LPE, SRC, true>(a); }

// the launch itself: tsim_launch.h (the plan: tsim_hip.hip ts_plan, TS_K_CLOSED_TANGENT)
template bool TsLaunch<void, false, float>::run_closed_tangent(const TsPlan&, hipStream_t, const TanClosedArgs<float>&);
template bool TsLaunch<void, false, double>::run_closed_tangent(const TsPlan&, hipStream_t, const TanClosedArgs<double>&);
