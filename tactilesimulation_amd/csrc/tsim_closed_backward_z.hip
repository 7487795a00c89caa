// tsim_closed_backward_z.hip — the GENERIC instantiations of k_closed_backward_z (tsim_kernels.h): the closed-loop adjoint kernel that also saves z of
// every sub-step, what tsim_push_closed_backward launches instead of the closed-loop k_backward while a table-gradient buffer is set
// (include/tsim.h tsim_set_param_grad; the parameter passes that read z: tsim_param_grad.hip, tsim_param_grad_body.hip).
// fp32 and fp64 at 16 / 32 / 64 lanes per environment, NRM 8 (tsim_launch.h ts_instantiated).  The two compiled-in twins (static:pusher,
// param:pusher: fp32, 16 lanes) are in tsim_static_pusher_policy.hip and tsim_param_pusher_policy.hip, with the closed-loop kernels of their view.
// A translation unit of its own, so that the kernels of tsim_hip.hip keep their code bytes and registers (the kernel table, host/buildhash.py);
// built like them: no fast-math flags, the fp64 instantiations follow the fp64 closed-loop adjoint to round-off.
// Also here, for the same reason: the kernel that writes the contact pass's frame -> seed-row table of such a launch (ts_closed_slots_launch).
#include <hip/hip_runtime.h>
#include "tsim_launch.h"

template bool TsLaunch<void, true, float>::run_closed_z(const TsPlan&, hipStream_t, const BwdArgs<float>&, float*);
template bool TsLaunch<void, true, double>::run_closed_z(const TsPlan&, hipStream_t, const BwdArgs<double>&, double*);

// Frame f of a closed-loop episode is observed by frame f + 1's policy call; the last frame's tactile output by nobody: slots[f] = f, and -1
// (no seed) for the last of the nframes.  With df_dtac = dobs_tac + one row, frame f then reads dobs_tac[f + 1] (PgArgs tac_slot, k_param_grad).
__global__ void __launch_bounds__(256) k_closed_slots(int32_t* slots, int nframes) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < nframes) slots[f] = f + 1 < nframes ? f : -1;
}
void ts_closed_slots_launch(int32_t* slots, int nframes, hipStream_t st) {
  hipLaunchKernelGGL(k_closed_slots, dim3((unsigned)((nframes + 255) / 256)), dim3(256), 0, st, slots, nframes);
}
