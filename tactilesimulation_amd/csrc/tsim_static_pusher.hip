// tsim_static_pusher.hip — the forward / adjoint kernels instantiated for the TactilePush model (envs/assets/pusher/pusher.xml) with its
// compiled blob as compile-time constants (tsim_static_pusher.h, generated; tsim_static.h: what that buys).  Its own translation unit because
// it is built with -ffinite-math-only -fno-signed-zeros — x * 0 -> 0, x + 0 -> x fold away the model's identity joint frames and unit axes —
// and the generic kernels (tsim_hip.hip) are not.  fp32, every launch shape (the debug kernel: four environments per wavefront, the shape of
// BASELINE.json's headline batch); built at -O2 (host/buildhash.py).  The closed-loop instantiations live in tsim_static_pusher_policy.hip.
// fp64 (round 5): the reference's arithmetic type (envs/tactile_push_env.py:29), two or one environments per wavefront — four do not fit the
// block's LDS in fp64.  The Newton systems are solved with partial pivoting there, as in every fp64 kernel (solve_newton).
// Which instantiations: tsim_launch.h ts_instantiated.
#include <hip/hip_runtime.h>
#include "tsim_launch.h"

template struct TsLaunch<TsStaticPusher, false, float>;
template struct TsLaunch<TsStaticPusher, false, double>;
