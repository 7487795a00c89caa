// tsim_static_pusher_policy.hip — the closed-loop instantiations of the static TactilePush kernels (the policy between the frames,
// tsim_policy_push.h): four environments per wavefront, the shape of BASELINE.json's headline batch.  Their own translation unit because they
// are built at -Os like the generic kernels: with the policy's layers inlined the forward kernel is 67 KB at -Os and 76 KB (512 registers,
// spills) at the -O2 the open-loop static kernels are built with (tsim_static_pusher.hip) — the instruction cache holds 64 KB.
// fp32 only (tsim_launch.h ts_instantiated): the fp64 view instantiates no kernel.
#include <hip/hip_runtime.h>
#include "tsim_launch.h"

template struct TsLaunch<TsStaticPusher, true, float>;
template struct TsLaunch<TsStaticPusher, true, double>;
