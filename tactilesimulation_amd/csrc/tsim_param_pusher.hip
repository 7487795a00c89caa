// tsim_param_pusher.hip — the forward / adjoint kernels instantiated for the STRUCTURE of the TactilePush model (envs/assets/pusher/pusher.xml):
// tree, joint types, contact pairs, dof / motor layout and the structural floats of the compiled asset (identity joint frames, unit axes,
// absent limits: TsParam<TsStaticPusher>::Fk) are compile-time constants, every other parameter is read from the batch's float records in LDS
// (tsim_static.h ts_F).  The fused register-resident evaluation (tsim_static_eval.h) as in tsim_static_pusher.hip, but for ANY batch with this
// structure: after tsim_update_model (the env's update_* randomisers) and with tsim_set_env_tables (one table per environment).  Same flags as the
// fully static unit: the folds are those of the structural entries.  Same instantiations too (tsim_launch.h ts_instantiated): fp32 at every
// launch shape, fp64 (round 5) at two or one environments per wavefront.
#include <hip/hip_runtime.h>
#include "tsim_launch.h"

template struct TsLaunch<TsParamPusher, false, float>;
template struct TsLaunch<TsParamPusher, false, double>;
