// tsim_param_pusher_policy.hip — the closed-loop instantiations (the policy between the frames, tsim_policy_push.h) of the STRUCTURE-static
// TactilePush kernels (tsim_param_pusher.hip: structure compiled in, parameters from the batch's float records, shared or per environment).
// Round 6: what lets the fused closed loop (include/tsim_env.h tsim_push_closed_rollout / _backward) stay on compiled-in kernels after the env's
// update_* edits and with one parameter table per environment (domain randomisation: envs/tactile_push_env.py has none, but
// envs/tactile_insertion_env.py:238-281 and envs/dclaw_rotate_env.py:169-178 draw theirs at every reset — a batched TactilePush collector does the same).
// Four environments per wavefront, fp32 only (tsim_launch.h ts_instantiated), built at -Os like tsim_static_pusher_policy.hip (the policy's layers
// inlined: the kernels are as large as the instruction cache).
#include <hip/hip_runtime.h>
#include "tsim_launch.h"

template struct TsLaunch<TsParamPusher, true, float>;
template struct TsLaunch<TsParamPusher, true, double>;
