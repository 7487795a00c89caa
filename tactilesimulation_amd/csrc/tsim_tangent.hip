// tsim_tangent.hip — the forward-mode tangent pass over the taped episode (include/tsim.h tsim_tangent_episode; the math: tsim_tangent.h).
//   k_tangent   slot = environment, 16 / 32 / 64 lanes as the adjoint launch, time runs FORWARDS over the tape.  Per sub-step the taped point is
//               evaluated once (link sweep with tangents, pairs, projection: K = dg/dq in c.H) and shared by all ndir directions; per direction one
//               K v, one M v, one solve with the taped Newton matrix (NOT transposed) and the contraction of the contact points' dF/dp with the
//               direction's parameters.  At a frame's end the directions' dq, dqd are written and pushed through the frame's outputs (the transpose of
//               output_vjp / vjp_taxels): the taxels evaluate the contact law once and emit every direction.
// Generic view only; a batch on a compiled-in model runs it over its own tape (the record stride includes K: TanArgs::tk) with its per-environment rows.
// It reads the tape and writes the caller's buffers, nothing else: the state, the carried adjoint and the pose records are not touched.
// Built like the generic kernels (tsim_hip.hip): no fast-math flags.  A unit of its own, so that no other kernel's code moves.
#include <hip/hip_runtime.h>
#include "tsim_kernels.h"
#include "tsim_tangent.h"
#include "tsim_tangent_kernel.h"
#include "tsim_launch.h"

template <class R, int NRM, bool EXPJ, int LPE>
__global__ void __launch_bounds__(TS_WAVE) k_tangent(TanArgs<R> a) { ts_tangent_walk<R, NRM, EXPJ, LPE, false>(a); }
// The body is tsim_tangent_kernel.h's ts_tangent_walk, and every edit of the kernel belongs there: k_tangent_src (tsim_tangent_body.hip) is the same
// body with SRC = true, and the two must not drift apart.

// the launch itself: tsim_launch.h, as every simulation kernel's (the plan: tsim_hip.hip ts_plan)
template bool TsLaunch<void, false, float>::run(const TsPlan&, hipStream_t, const TanArgs<float>&);
template bool TsLaunch<void, false, double>::run(const TsPlan&, hipStream_t, const TanArgs<double>&);
