/* tsim.h — C ABI of the MI355X-native batched tactile-simulation step (libtsim_hip.so).
 *
 * This is the drop-in boundary for ONE path of eanswer/TactileSimulation: what its python layer calls on
 * `redmax_py.Simulation` (pybind11 over the un-vendored DiffRedMax C++) from
 * envs/redmax_torch_functions.py.  Every entry point below names the reference call it replaces
 * (paths relative to the reference repo).  Plain pointers and sizes only — no torch types.
 *
 * One `tsim_batch` = B independent environments of one model, resident on one GPU.  The reference's
 * one-environment `Simulation` object is B = 1.  All array arguments are DEVICE pointers of the batch's
 * real type (float for TSIM_F32, double for TSIM_F64), env-major ([B][dim], C order) unless noted.
 * TSIM_F32 batches are mixed precision inside: positions, link poses and penetration depths are double, everything
 * else float; the interface stays float.
 * `stream` is a hipStream_t (NULL = default stream).  Functions return 0 on success, non-zero on error
 * (message via tsim_last_error()).  Calls on one batch must be serialised by the caller (the reference's
 * Simulation is single-threaded as well: algorithms/gd.py:30 torch.set_num_threads(1)).
 */
#ifndef TSIM_H
#define TSIM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct tsim_batch tsim_batch;
enum { TSIM_F32 = 0, TSIM_F64 = 1 };

/* redmax.Simulation(model_path)                       envs/redmax_torch_env.py:33
 * The XML is compiled on the host (tactilesimulation_amd/model/compiler.py) to the flat blob of
 * include/tsim_blob.h; I / F are HOST pointers.  tape_capacity = max number of recorded sub-steps
 * between reset() and backward (TactilePush: 100 env-steps x 5 = 500). */
int tsim_batch_create(const int32_t* I, const double* F, int B, int tape_capacity, int dtype, int device,
                      tsim_batch** out);
void tsim_batch_destroy(tsim_batch* b);

/* sim.ndof_r / ndof_u / ndof_var / ndof_tactile / options.h   envs/redmax_torch_env.py:35-37,
 * envs/redmax_torch_functions.py:161, envs/tactile_push_env.py:67 */
int tsim_ndof_r(const tsim_batch* b);
int tsim_ndof_u(const tsim_batch* b);
int tsim_ndof_var(const tsim_batch* b);
int tsim_ndof_tactile(const tsim_batch* b);
int tsim_batch_size(const tsim_batch* b);
int tsim_dtype(const tsim_batch* b);
double tsim_timestep(const tsim_batch* b);
int tsim_tape_len(const tsim_batch* b);          /* recorded sub-steps since the last reset */

/* update_* model edits (envs/dclaw_rotate_env.py:173-178, envs/tactile_insertion_env.py:254-279,
 * envs/stable_grasp_env.py:122): the host recompiles the blob and re-uploads it.  Topology (counts,
 * offsets) must be unchanged. */
int tsim_update_model(tsim_batch* b, const int32_t* I, const double* F, void* stream);

/* Batched counterpart of the update_* randomisers (envs/tactile_insertion_env.py:238-281 draws new contact / tactile
 * parameters per episode; with B environments each one gets its own): `tables` is a DEVICE array [B][tsim_table_size]
 * of the batch's real type whose rows are copies of the leading `tsim_table_size` reals of the blob's F[] (all numeric
 * tables: links, dofs, motors, variables, pairs, sensors) with the randomised entries overwritten. NULL reverts to the
 * shared model. Point arrays (contact points, taxels) are always shared.  The float header of a row (time step, gravity, Newton tolerance:
 * F[0 .. TSIM_FH_SIZE)) is NOT per environment: it is overwritten with the shared model's (the reference's randomisers never touch it).
 * On an fp32 batch whose model has a compiled-in structure this call checks on the device that every row keeps it and reads one int back: it
 * synchronises `stream` then.  Inside a stream capture the check cannot run: the batch then takes the generic kernels for as long as these tables
 * are set (tsim_kernel_variant says so) — set the tables before capturing to keep the compiled-in instantiation in the graph. */
int tsim_set_env_tables(tsim_batch* b, const void* tables, void* stream);
int tsim_table_size(const tsim_batch* b);

/* backward_info.flag_p / backward_results.df_dp (envs/redmax_torch_functions.py:83,151), batched, for the physical parameters
 * of the numeric tables: while dL_dtables (DEVICE [B][tsim_table_size], the batch's real type) is set, every tsim_backward_steps /
 * tsim_backward_episode ADDS dL/d(row entry) for the entries tsim_model_table_offset names (pair kn kt mu damping, sensor kn kt mu
 * damping, dof damping) and leaves every other entry untouched.  NULL = off.  No host synchronisation.
 * Per environment: dL/dp = sum over the undone sub-steps t of -(dg_t/dp)^T z_t (g_t = r_t / ca_t the scaled residual, z_t the adjoint
 * solution of the sub-step) + the direct term of the seeded tactile frames (sensor parameters).  The adjoint launch then saves z of every
 * sub-step (the same kernel variant, compiled with that store) and a second pass over (environment, chunk of sub-steps) adds the gradient;
 * sums are in a fixed order (bit-identical from run to run).  The entries are those of the environment's row of tsim_set_env_tables, or of
 * the shared model.  The stick / slip switch of the friction law is a kink: these are one-sided derivatives of the smooth piece each contact
 * point is on (tsim_debug_signature).  The first non-NULL call allocates [tape_capacity][B][ndof_r] reals for z.  The fused closed-loop
 * adjoint launch (include/tsim_env.h tsim_push_closed_backward) adds to the buffer in the same way, under the same conventions.
 * While the buffer is NULL nothing more is launched or allocated by any adjoint launch, and the kernels that run are the ones that ran before. */
int tsim_set_param_grad(tsim_batch* b, void* dL_dtables);

/* Which groups of table entries tsim_set_param_grad's buffer receives (a mask of TSIM_PG_*; the default, TSIM_PG_CONTACT, is the list above):
 *   TSIM_PG_INERTIAL  per link: mass, centre of mass (3, link frame), inertia about it (6: xx yy zz xy xz yz, link frame) — TSIM_TAB_LINK.
 *                     g_j contains W_j . sum_{i in subtree(j)} F_i / ca, F_i = I_i A_i + V_i x* I_i V_i the link's inertial wrench (gravity is the
 *                     world's acceleration), so the term is -(Z_i . dF_i/dp) / ca with Z_i = sum_{j above i} z_j W_j; the sub-step's discrete
 *                     accelerations are those of the adjoint.  Massless intermediate links of a free3d-* joint get their derivative too.
 *   TSIM_PG_MOTOR     per entry of u: lo hi P D — TSIM_TAB_MOTOR.  Force control: d tau/d lo = 1 - s, d tau/d hi = s, s = (clip(u, -1, 1) + 1) / 2,
 *                     P and D exactly 0; position control: d tau/d P = u - q, d tau/d D = -qd, lo and hi exactly 0.
 *   TSIM_PG_LIMIT     per dof: lim_lo lim_hi lim_k — TSIM_TAB_LIMIT; the one-sided derivative of the piece the state is on, exactly 0 inside
 *                     the limits and for a dof without a limit (lim_k == 0).
 * Host-side only; takes effect with the next adjoint launch.  With the default mask nothing more is launched or allocated and every result is
 * bit-identical; a body group adds one pass over (environment, chunk of sub-steps) and its fixed-order reduction (csrc/tsim_param_grad_body.hip
 * k_param_grad_body).  Without TSIM_PG_CONTACT the contact, tactile and damping columns are left untouched.
 * Not differentiated, by design: geometry (joint frames and axes, primitive frames and shapes, contact points, taxels, end-effector
 * positions), the float header (time step, gravity, tolerance), and the B = 1 redmax_py shim's flag_p. */
enum { TSIM_PG_CONTACT = 1, TSIM_PG_INERTIAL = 2, TSIM_PG_MOTOR = 4, TSIM_PG_LIMIT = 8 };
int tsim_set_param_grad_groups(tsim_batch* b, int mask);
int tsim_get_param_grad_groups(const tsim_batch* b);      /* the mask (-1: null batch) */

/* Diagnostics: what the most recent adjoint launch of the batch ran.  out[0]: its kernel (TSIM_ADJ_*; -1: no adjoint launch yet) — k_backward,
 * its twin that also saves z (a buffer was set: tsim_set_param_grad), or the closed-loop adjoint's twin (tsim_push_closed_backward with a buffer
 * set); out[1]: the parameter passes launched behind it, bit 0 the contact pass (k_param_grad), bit 1 the body groups' (k_param_grad_body). */
enum { TSIM_ADJ_BACKWARD = 0, TSIM_ADJ_BACKWARD_Z = 1, TSIM_ADJ_CLOSED_BACKWARD_Z = 2 };
int tsim_last_adjoint_launch(const tsim_batch* b, int32_t* out);

/* sim.set_state_init(q, qdot) + sim.reset(backward_flag)      envs/redmax_torch_functions.py:39-41,
 * envs/tactile_push_env.py:138,154.  q0 / qd0: [B][ndof_r].  Restarts the tape and zeroes the carried
 * adjoint. */
int tsim_reset(tsim_batch* b, const void* q0, const void* qd0, int backward_flag, void* stream);

/* The same for the environments with mask[env] != 0 only (DEVICE int32[B]); the others keep their state.  This is what
 * a batched roll-out collector does when single episodes end (the reference resets one `Simulation` at a time:
 * envs/dclaw_rotate_env.py:181-199 reset() per env).  Forward-only batches only: the tape is shared by the batch.  On a
 * BDF2 model the environment restarts with a constant-velocity history (q_-1 = q0 - h qd0). */
int tsim_reset_masked(tsim_batch* b, const void* q0, const void* qd0, const int32_t* mask, void* stream);

/* sim.set_u(u); sim.forward(num_steps, ...); sim.get_q(); sim.get_variables();
 * sim.get_tactile_force_vector()                               envs/redmax_torch_functions.py:131-136
 * (and :48-57 with num_steps = 1).  u: [B][ndof_u], held for num_steps implicit sub-steps.
 * Outputs (any may be NULL): q_out, qd_out [B][ndof_r]; var_out [B][ndof_var]; tac_out [B][ndof_tactile]
 * (taxel-major: shear0, shear1, normal); status [B] int32 = number of sub-steps whose Newton solve did not
 * reach tol (bit 30 set if a non-finite value appeared, in the state or in u: a NaN / inf control is flagged here rather than
 * swallowed by the motor law's clamp). */
int tsim_step(tsim_batch* b, const void* u, int num_steps, void* q_out, void* qd_out, void* var_out,
              void* tac_out, int32_t* status, void* stream);

/* sim.get_q() / get_qdot() / get_variables() / get_tactile_force_vector() at the current state, e.g.
 * right after reset (envs/tactile_push_env.py:157) or after forward() where the pad is too large to be read out inside the step
 * (examples/RollingBallExp/test_sim_speed.py:77-80: 40 000 taxels).  tsim_readout is two launches — kinematics of the current state,
 * then one kernel whose lanes are taxels — or, for pads of >= 4096 taxels right after a forward launch, the second one alone: that
 * launch leaves the pose records of the state it ends in.  Same results either way, and the same bits as the tactile frames tsim_step /
 * tsim_rollout write — to round-off where a sensor has more than four primitives and the launch reads out inside the stepping kernel
 * (closed-loop launches, launches under capture, TSIM_INKERNEL_READOUT=1, more than 64 (sensor, primitive) combinations or 16 sensors):
 * that read-out stages a sensor's primitives in groups of four and adds the taxel's projected outputs group by group, where the taxel
 * kernels add the forces and project once (measured 5e-8 of the frame's maximum in fp32, 1e-16 in fp64, on a taxel that two groups load:
 * tests/test_gpu_tactile_readout_shapes.py).  Any other change of state (reset, masked reset,
 * new model tables, cache pop) and any HIP-graph capture of this batch's launches switch back to two. */
int tsim_get_state(tsim_batch* b, void* q_out, void* qd_out, void* stream);
int tsim_readout(tsim_batch* b, void* var_out, void* tac_out, void* stream);

/* backward_info.set_flags / df_dq / df_dvar / df_dtactile; sim.backward_steps(n);
 * backward_results.df_du                                       envs/redmax_torch_functions.py:151-170
 * Adjoint of the newest n recorded sub-steps, newest first, continuing the adjoint carried from earlier
 * calls; pops them from the tape.
 *   seed_mode 0: df_dq [B][ndof_r], df_dvar [B][ndof_var], df_dtac [B][ndof_tactile] are the partials w.r.t.
 *                the outputs after the LAST of the n sub-steps (what StepSimFunction.backward builds by
 *                zero-padding, :153-163);
 *   seed_mode 1: [B][n][dim], step-major, oldest first (the general layout of the reference).
 * Any seed pointer may be NULL (= zeros).  df_du: [B][n][ndof_u], oldest first (reshape(num_steps, ndof_u)
 * at :170). */
int tsim_backward_steps(tsim_batch* b, int n, int seed_mode, const void* df_dq, const void* df_dvar,
                        const void* df_dtac, void* df_du, void* stream);

/* The open-loop episode of EpisodicSimFunction.forward             envs/redmax_torch_functions.py:46-57
 *   for t in range(T): sim.set_u(actions[t]); sim.forward(n); q, variables = getters;
 *                      if tactile_masks[t]: tactile = get_tactile_force_vector()
 * as ONE launch: frame f applies u[f] for num_steps sub-steps and writes its outputs to slot f.
 *   u [num_frames][B][ndof_u];  q_out, qd_out [num_frames][B][ndof_r], var_out [num_frames][B][ndof_var],
 *   tac_out [num_masked][B][ndof_tactile] (any may be NULL);  status [B]: non-converged sub-steps of the whole call.
 *   tactile_slot: DEVICE int32[num_frames], slot of frame f in tac_out or < 0 for "no tactile read-out at this frame"
 *   (the tactile_masks of :55-57 as an exclusive prefix count); NULL = every frame, slot f.
 * Results are bit-identical to num_frames calls of tsim_step; no environment waits for the slowest one of the batch
 * between env-steps, which is where the per-step launches lose their time. */
int tsim_rollout(tsim_batch* b, const void* u, int num_frames, int num_steps, const int32_t* tactile_slot,
                 void* q_out, void* qd_out, void* var_out, void* tac_out, int32_t* status, void* stream);

/* sim.backward() of EpisodicSimFunction.backward                  envs/redmax_torch_functions.py:77-92
 * Adjoint of the newest num_frames * num_steps sub-steps in one launch.  Seeds are the partials w.r.t. the outputs of
 * each frame (time-major like tsim_rollout's outputs): df_dq [num_frames][B][ndof_r], df_dvar [num_frames][B][ndof_var],
 * df_dtac [num_masked][B][ndof_tactile] (tactile_slot as in tsim_rollout), any may be NULL.
 * df_du [num_frames][B][ndof_u] = gradient w.r.t. u[f]
 * (summed over the frame's sub-steps).  Continues / leaves the carried adjoint like tsim_backward_steps. */
int tsim_backward_episode(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot,
                          const void* df_dq, const void* df_dvar, const void* df_dtac, void* df_du, void* stream);

/* Forward-mode tangent pass (no reference counterpart): the derivative of the outputs of the newest num_frames * num_steps taped sub-steps along
 * ndir directions at once (1 .. TSIM_TANGENT_MAX_DIR) — J v where tsim_backward_episode + tsim_get_adjoint + tsim_set_param_grad give J^T w.
 * It reads the tape and writes the caller's buffers, nothing else: the tape is not popped, the state, the carried adjoint, the cache and the pose
 * records are not touched; it may be called any number of times between a recorded roll-out and its adjoint, which afterwards returns the bits it
 * would have returned without the calls.  No host synchronisation and no allocation, with one exception: with a body group on and dtables
 * given, the body columns' part of the sources is computed into a workspace of the batch, [ndir][num_frames * num_steps][B][ndof_r] reals, which
 * grows only.  The first call that needs it, or needs it larger, allocates it and synchronises the stream; later calls of the same or a smaller
 * size do neither.  A call that would have to allocate under stream capture is refused: capture a launch only after a warm-up call of that
 * size.  A workspace that a captured graph names is kept until the batch is destroyed, so a replay after a later, larger call stays valid.  The
 * workspace is freed with the batch; nothing is allocated while no body group is on.  Because it belongs to the batch, tangent calls of one batch
 * that read body columns must be issued on one stream, or be ordered by the caller: two of them in flight at once would share it.
 * Inputs (device memory, the batch's real type; NULL = zeros), direction outermost:
 *   du [ndir][num_frames][B][ndof_u];  dq0, dqd0 [ndir][B][ndof_r]: the tangent of the state at the window's start;
 *   dtables [ndir][B][tsim_table_size]: the TSIM_PG_CONTACT columns are always read (contact pair and sensor kn kt mu damping, dof damping),
 *   and with them the columns of every body group that is on in the batch's tsim_set_param_grad_groups mask — TSIM_PG_INERTIAL: link mass,
 *   centre of mass, inertia; TSIM_PG_MOTOR: motor lo hi P D; TSIM_PG_LIMIT: dof limit lo hi k (the TSIM_TAB_LINK / MOTOR / LIMIT columns).
 *   Every other entry is not read at all.  With the default mask (TSIM_PG_CONTACT) a body column changes no output bit; with a body group on
 *   and dtables NULL or zero on its columns the outputs are those of the default mask, bit for bit (the body term adds exact zeros).
 * Outputs (NULL = not written), time-major like tsim_rollout's with the direction outermost:
 *   dq_out, dqd_out [ndir][num_frames][B][ndof_r];  dvar_out [ndir][num_frames][B][ndof_var];
 *   dtac_out [ndir][num_masked][B][ndof_tactile] (tactile_slot as in tsim_rollout).
 * Per BDF1 sub-step, with H the taped Newton matrix of the accepted iterate, K = dg/dq at it, M the mass matrix, D du the motor term
 * (dtu / ca on the motor's dof; a clipped force control has none) and g = r / ca:
 *     s = -K dq0 + h M dqd0 + D du - (dg/dp) dp ,   H y = s ,   dq1 = dq0 + y ,   dqd1 = cv y
 * — the exact transpose of the adjoint launches (rhs = lam_q + cv lam_v; H^T z = rhs; lam_q' = lam_q - K^T z; lam_v' = h M z; dL/du = D^T z;
 * dL/dp = -(dg/dp)^T z), so a sub-step that did not converge is treated as the adjoint treats it, and the stick / slip switch and the joint
 * limits give the one-sided derivative of the piece each point is on.  BDF2 sub-steps (tape record >= 2) carry the tangents of the two states
 * before them: kv = -4/3 dq0 + 1/3 dq_1, mv = 8h/9 dqd0 - 2h/9 dqd_1, s = K kv + M mv + ..., dq1 = y - kv.  At a frame's end dq, dqd are
 * written, dvar = J_var dq, and every loaded taxel emits A^T R_PA^T (Jx dx + Jv dxd - dth x F + dF/dp_sensor dp); an unloaded taxel an exact 0.
 * The body columns enter a sub-step's source only through the residual, -(dg/dp) dp linearised at the taped state (the transpose of the body
 * groups' gradient): per link dF_i = dI_i A_i + V_i x* dI_i V_i for the direction's mass, centre of mass and inertia, with the sub-step's discrete
 * acceleration as the gradient pass forms it, and s_j -= W_j . (sum of dF_i over the subtree of dof j) / ca, massless intermediate links of a
 * free3d joint included; per motor s_j += dtau / ca on its dof, dtau = (1 - c) dlo + c dhi with c = (clip(u, -1, 1) + 1) / 2 under force control
 * (P, D: exactly 0), dtau = (u - q) dP - qd dD under position control (lo, hi: exactly 0); per dof the one-sided derivative of the limit spring's
 * piece (exactly 0 inside the limits and for k = 0).  A pass of its own (k_tangent_body_src) computes this for all sub-steps before k_tangent.
 * Parameters are the environment's row of tsim_set_env_tables, or the shared model's.  Directions are independent: a direction's bits do
 * not depend on ndir or on the other directions.
 * Returns non-zero (tsim_last_error) and launches nothing for: a null batch; ndir outside 1 .. 8; no tape recorded or a window longer than the
 * tape; a BDF2 model whose window does not start at tape record 0 (no tangent is carried across calls).
 * The fused closed loop has its own entry point, tsim_push_closed_tangent (tsim_env.h): the same sub-steps, a frame's du from the policy's tangent.
 * Out of scope: geometry and the float header as directions; the B = 1 shim; torch forward-mode AD. */
enum { TSIM_TANGENT_MAX_DIR = 8 };
int tsim_tangent_episode(tsim_batch* b, int num_frames, int num_steps, int ndir, const int32_t* tactile_slot,
                         const void* du, const void* dq0, const void* dqd0, const void* dtables,
                         void* dq_out, void* dqd_out, void* dvar_out, void* dtac_out, void* stream);
/* Diagnostics: the static launch geometry of a tsim_tangent_episode call of ndir directions (with_dtables: dtables given), as tsim_launch_info
 * reports the forward / backward kernels': out[0] = LDS bytes per block (the contexts and the launch's tangent blocks), out[1] = threads per
 * block, out[2] = blocks, out[3] = lanes per environment.  The lanes are the batch's (tsim_launch_info), doubled until a block holds the tangent
 * state of TSIM_TANGENT_MAX_DIR directions with parameters, so they do not depend on ndir or with_dtables; the LDS bytes do. out = int32[4]. */
int tsim_tangent_launch_info(const tsim_batch* b, int ndir, int with_dtables, int32_t* out);

/* Per-frame transition Jacobians (no reference counterpart): the local linearisation of the dynamics over the newest num_frames * num_steps taped
 * sub-steps, every frame in ONE launch.  Frame f is sub-steps f * num_steps .. (f + 1) * num_steps - 1 of that window; with x = (q, qdot):
 *   A_out    [num_frames][B][2 ndof_r][2 ndof_r]   dx_{f+1} / dx_f: rows (q, qdot) at the frame's end, columns (q, qdot) at its start;
 *   B_out    [num_frames][B][2 ndof_r][ndof_u]     dx_{f+1} / du_f, u held for the frame's sub-steps; a clipped force control: exactly zero columns;
 *   Jvar_out [num_frames][B][ndof_var][ndof_r]     dvariables / dq at the frame's END state, the measurement map that goes with x_{f+1}
 *                                                  (tsim_tangent_episode's dvar = Jvar dq).
 * Device memory, the batch's real type, row-major; any may be NULL (not written); with A_out and B_out both NULL nothing is solved.  So
 * x_{f+1} = A_f x_f + B_f u_f to first order, and chaining the frames reproduces tsim_tangent_episode's dq, dqd to round-off.
 * Per sub-step it is tsim_tangent_episode's BDF1 recursion seeded with the identity, for all 2 ndof_r + ndof_u columns:
 *     s = -K dq0 + h M dqd0 + D du ,   H y = s ,   dq1 = dq0 + y ,   dqd1 = cv y
 * with H the taped Newton matrix and K, M, D of the taped point, evaluated once for all columns; the columns are solved eight per elimination of H
 * (in double, with partial pivoting).  A sub-step that did not converge is treated as the adjoint treats it; limits and stick / slip give the
 * one-sided derivative of the piece the state is on.  Parameters are the environment's row of tsim_set_env_tables, or the shared model's.  A
 * frame's matrices depend on that frame's tape records only: their bits depend neither on num_frames nor on which outputs are given (A, B).
 * Read-only: the tape is not popped; the state, the carried adjoint, the cache and the pose records are untouched.  No allocation, no host
 * synchronisation; capturable.  A compiled-in model's batch runs the generic evaluation on its tape, as tsim_tangent_episode does.
 * Returns non-zero (tsim_last_error) and launches nothing for: a null batch; no tape recorded or a window longer than the tape; num_frames or
 * num_steps < 1; a BDF2 model (its transition acts on two states of history); a model whose block would not fit the 64 KB of LDS.
 * Out of scope: geometry as inputs; BDF2; the B = 1 shim; the fused closed-loop tape.  (The tactile Jacobian, ndof_tactile x 2 ndof_r per frame
 * and environment, has its own entry: tsim_tactile_jacobians below; so have the contact-group table columns as inputs: tsim_param_jacobians.) */
int tsim_frame_jacobians(tsim_batch* b, int num_frames, int num_steps, void* A_out, void* B_out, void* Jvar_out, void* stream);
/* Diagnostics: the static launch geometry of a tsim_frame_jacobians call, as tsim_tangent_launch_info reports a tangent call's: out[0] = LDS bytes
 * per block (the contexts and the slots' column blocks), out[1] = threads per block, out[2] = blocks PER FRAME, out[3] = lanes per environment:
 * the batch's, doubled until a block fits 64 KB; they do not depend on which outputs are asked for.  out = int32[4]. */
int tsim_frame_jacobians_launch_info(const tsim_batch* b, int32_t* out);

/* Per-frame tactile Jacobians (no reference counterpart): C_f = dtactile / dx, x = (q, qdot), of every MASKED frame of the newest num_frames *
 * num_steps taped sub-steps, in ONE launch.  The window and tactile_slot are tsim_rollout's / tsim_tangent_episode's (DEVICE int32[num_frames],
 * slot of frame f in Ct_out or < 0: frame not wanted; NULL: slot f).
 *   Ct_out [num_masked][B][2 ndof_r][ndof_tactile]   the TRANSPOSE of C_f: row d is column d of C_f stored as one contiguous tactile frame (the
 *                                                    layout of tsim_tangent_episode's dtac_out[d]); rows d < ndof_r are dtactile / dq_d, rows
 *                                                    ndof_r + d are dtactile / dqdot_d.  Device memory, the batch's real type.
 * It is large: 2 ndof_r * ndof_tactile reals per environment and masked frame (TactilePush, fp32: 21 840 bytes; D'Claw: 217 440 bytes).
 * C_f is the Jacobian of the read-out map tac(q, qdot) at the frame's END state, q and qdot taken as independent variables.  So
 * dtac_f = C_f dx_{f+1}, and with tsim_frame_jacobians' matrices C_f A_f and C_f B_f are the tactile response to the frame's start state and to
 * its control; dtactile / du itself is zero.  Every loaded taxel emits, per column, A^T R_PA^T (Jx dx + Jv dxd - dth x F) with dx = dth x x + drho,
 * dxd = dv + dw x x + wrel x dx and (dth, drho, dw, dv) the pair's record of the column's dof: tsim_tangent_episode's expression for a unit
 * direction, without the parameter term.  At a stick / slip switch or a surface edge that is the one-sided derivative of the piece the taxel is
 * on, as the adjoint and the tangent take it.  An unloaded taxel, and a sensor without primitives, give exact zero rows of C_f.  Parameters are
 * the environment's row of tsim_set_env_tables, or the shared model's.  BDF2 and rotation-vector models are accepted: only the (q, qdot) of the
 * frame's last tape record is read, nothing is solved.  A frame's bits depend neither on num_frames, nor on the mask, nor on the environment's
 * position in the batch or the batch size.
 * Read-only: the tape is not popped; the state, the carried adjoint, the cache and the pose records are untouched.  No allocation, no host
 * synchronisation; capturable.  A compiled-in model's batch runs the generic evaluation on its tape, as tsim_tangent_episode does.
 * Returns non-zero (tsim_last_error) and launches nothing for: a null batch or a null Ct_out; no tape recorded or a window longer than the tape;
 * num_frames or num_steps < 1; a model without taxels; a model whose block would not fit the 64 KB of LDS; more than 2^31 - 1 blocks.  The mask is
 * device memory, which this call does not read on the host: with no masked frame every block returns at once and nothing is written (the Python
 * layer, which builds the mask, refuses such a call).
 * Out of scope: geometry as inputs; the fused closed-loop tape; the B = 1 shim.  (The contact-group table columns as inputs, F_f = dtactile / dp,
 * have their own entry: tsim_param_jacobians below; so have the products H^T W H and H^T W r of H = [C_f | F_f], which never store C_f:
 * tsim_tactile_normal_equations.) */
int tsim_tactile_jacobians(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot, void* Ct_out, void* stream);
/* Diagnostics: the static launch geometry of a tsim_tactile_jacobians call, as tsim_frame_jacobians_launch_info reports: out[0] = LDS bytes per
 * block (the contexts and the slots' record blocks), out[1] = threads per block, out[2] = blocks PER FRAME, out[3] = lanes per environment: the
 * batch's, doubled until a block fits 64 KB.  out = int32[4]. */
int tsim_tactile_jacobians_launch_info(const tsim_batch* b, int32_t* out);

/* Per-frame parameter Jacobians (no reference counterpart): the missing block of the local linearisation of a taped episode,
 *     x_{f+1} ~ A_f x_f + B_f u_f + E_f p ,      tactile_f ~ C_f x_{f+1} + F_f p ,      x = (q, qdot),
 * for every frame of the newest num_frames * num_steps taped sub-steps in ONE launch (A, B: tsim_frame_jacobians; C: tsim_tactile_jacobians).
 * p is the environment's contact-group parameters, the columns tsim_set_param_grad differentiates: per contact pair and per tactile sensor
 * kn kt mu damping, per dof its damping.
 *   cols    HOST int32[ncols]: the table columns wanted in E (column indices of a tsim_table_size row; 1 .. TSIM_PARAM_JACOBIAN_MAX_COLS of
 *           them, each once).  Read during the call and passed to the kernel by value; a caller who wants more columns launches again.
 *   E_out   [num_frames][B][2 ndof_r][ncols]   E_f = dx_{f+1} / dp at fixed (x_f, u_f): rows (q, qdot) at the frame's end, column k = cols[k].
 *   Ft_out  [num_masked][B][4][ndof_tactile]   F_f = dtactile / dp at fixed x_{f+1}, stored compactly: a taxel belongs to ONE sensor, so row k
 *           (k = kn, kt, mu, damping) holds the derivative of every taxel w.r.t. field k of ITS OWN sensor, as one contiguous tactile frame (the
 *           layout of Ct_out's rows).  The dense F_f (ndof_tactile x 4 nsensor) is that row scattered by sensor; pair and dof-damping columns
 *           have no direct tactile term.  tactile_slot is tsim_tactile_jacobians' DEVICE mask (NULL: slot f); it is used for Ft_out only.
 * Device memory, the batch's real type, row-major; either output may be NULL (not written), not both.
 * E is tsim_tangent_episode's BDF1 recursion over the frame's sub-steps for unit dtables columns, every column starting at zero:
 *     s_col = -K dq0_col + h M dqd0_col - dg/dp_col ,   H y = s ,   dq1 = dq0 + y ,   dqd1 = cv y
 * with H the taped Newton matrix and K of the taped point, evaluated once for all columns, and M dqd0 the tangent pass's own product per column; the
 * columns are solved eight per elimination of H.  dg/dp_col is the tangent pass's: for a pair column the pair's wrench derivative on every dof above its links, for a dof's damping
 * qdot_j / ca on that dof.  Exact zeros: a sensor column (sensors do not enter the dynamics), a sensing-only pair, and a pair that is near in no
 * sub-step of the frame, give an exactly zero column of E; an unloaded taxel and a sensor without primitives give exact zeros in Ft.
 * With E_out NULL nothing is solved: only the frame's last record is evaluated, and BDF2 and rotation-vector models are accepted, as
 * tsim_tactile_jacobians accepts them.  Parameters are the environment's row of tsim_set_env_tables, or the shared model's.  A column's bits
 * depend neither on the other columns listed nor on its position in cols, nor on num_frames, on whether Ft_out is given, or on the batch size.
 * Read-only: the tape is not popped; the state, the carried adjoint, the cache and the pose records are untouched.  No device copy, no
 * allocation, no host synchronisation; capturable.  A compiled-in model's batch runs the generic evaluation on its tape.
 * Returns non-zero (tsim_last_error) and launches nothing for: a null batch; both outputs NULL; E_out with ncols < 1 or >
 * TSIM_PARAM_JACOBIAN_MAX_COLS or null cols; a column that is not a contact-group parameter (body-group columns, geometry, the float header); a
 * column listed twice; Ft_out on a model without taxels; no tape recorded or a window longer than the tape; num_frames or num_steps < 1; E_out on a
 * BDF2 model; a model whose block would not fit the 64 KB of LDS; more than 2^31 - 1 blocks.
 * Scope: contact-group columns only.  Out of scope: the body groups (link inertia, motors, limits) and geometry as columns; the fused closed-loop
 * tape; the B = 1 shim; more than TSIM_PARAM_JACOBIAN_MAX_COLS columns per launch. */
enum { TSIM_PARAM_JACOBIAN_MAX_COLS = 32 };
int tsim_param_jacobians(tsim_batch* b, int num_frames, int num_steps, int ncols, const int32_t* cols,
                         const int32_t* tactile_slot, void* E_out, void* Ft_out, void* stream);
/* Diagnostics: the static launch geometry of a tsim_param_jacobians call, as tsim_frame_jacobians_launch_info reports: out[0] = LDS bytes per
 * block (the contexts and the slots' column blocks, sized for TSIM_PARAM_JACOBIAN_MAX_COLS columns), out[1] = threads per block, out[2] = blocks
 * PER FRAME, out[3] = lanes per environment: the batch's, doubled until a block fits 64 KB; they depend neither on ncols nor on which outputs are
 * asked for.  out = int32[4]. */
int tsim_param_jacobians_launch_info(const tsim_batch* b, int32_t* out);

/* Tactile normal equations (no reference counterpart): the information form of the tactile block of a taped episode's linearisation,
 *     N_f = H_f^T W H_f ,      n_f = H_f^T W r_f ,      H_f = [C_f | F_f]   (ndof_tactile x Z),   Z = 2 ndof_r + (with_params ? 4 nsensor : 0),
 * for every masked frame of the newest num_frames * num_steps taped sub-steps in ONE launch, without C_f or F_f ever being stored: what an
 * information filter (info = P^-1 + H^T R^-1 H, eta = P^-1 z + H^T R^-1 y) and Gauss-Newton / LM on tactile residuals consume.  C_f is exactly
 * tsim_tactile_jacobians' C_f (x = (q, qdot) at the frame's END state); F_f is the dense form of tsim_param_jacobians' compact Ft: column
 * 2 ndof_r + 4 s + k is field k (kn, kt, mu, damping) of sensor s, non-zero only on that sensor's taxels.  The window and tactile_slot are
 * tsim_tactile_jacobians' (a DEVICE int32 mask; NULL: slot f).
 *   weight  DEVICE [ndof_tactile] or NULL (ones): the diagonal of W, an inverse variance per tactile value, shared by all environments and
 *           frames.  It is not read on the host: negative or non-finite weights are the caller's business (they enter the sums as they are, on
 *           the loaded taxels only).
 *   resid   DEVICE [num_masked][B][ndof_tactile] or NULL: r.
 *   N_out   [num_masked][B][Z][Z], dense, row-major, EXACTLY symmetric (an entry is computed once and mirrored).  Not NULL.
 *   n_out   [num_masked][B][Z]; given if and only if resid is.
 * Device memory, the batch's real type.  Z^2 + Z reals per environment and masked frame: TactilePush with parameters, fp32: 1 368 bytes, where
 * Ct and Ft together are 27 300.  r^T W r is not computed (it needs the unloaded taxels too).
 * A taxel's rows are summed over its sensor's primitives BEFORE the product.  The sums run over the loaded taxels in ascending order, one fixed
 * order at every launch shape, without atomics: a frame's bits depend neither on num_frames, nor on the mask, nor on the batch size or the
 * environment's position in the batch; the state block N[:2 ndof_r, :2 ndof_r] and n[:2 ndof_r] have the same bits with and without with_params,
 * and N with and without resid.  Exact zeros: a frame in which no taxel is loaded gives all-zero N and n; a sensor without primitives or
 * without a loaded taxel exactly zero parameter rows and columns; the blocks between two sensors' parameter columns are exactly zero.  Every
 * entry of both outputs is written on every call.  Parameters are the environment's row of tsim_set_env_tables, or the shared model's.  BDF2 and
 * rotation-vector models are accepted: only the (q, qdot) of the frame's last tape record is read, nothing is solved.
 * Read-only: the tape is not popped; the state, the carried adjoint, the cache and the pose records are untouched.  No device copy, no
 * allocation, no host synchronisation; capturable.  A compiled-in model's batch runs the generic evaluation on its tape.
 * Returns non-zero (tsim_last_error) and launches nothing for: a null batch or a null N_out; exactly one of resid and n_out given; no tape
 * recorded or a window longer than the tape; num_frames or num_steps < 1; a model without taxels; a model whose block would not fit the 64 KB of
 * LDS; more than 2^31 - 1 blocks.  With no masked frame in the device mask every block returns at once and nothing is written.
 * Out of scope: a full (non-diagonal) W; r^T W r; the pair and dof-damping columns (no direct tactile term: exact zeros, which
 * functions.episode_information fills in); the fused closed-loop tape; the B = 1 shim. */
int tsim_tactile_normal_equations(tsim_batch* b, int num_frames, int num_steps, const int32_t* tactile_slot, int with_params,
                                  const void* weight, const void* resid, void* N_out, void* n_out, void* stream);
/* Diagnostics: the static launch geometry of a tsim_tactile_normal_equations call, as tsim_frame_jacobians_launch_info reports: out[0] = LDS
 * bytes per block (the contexts, the slots' records, sums and row tiles, the entry table), out[1] = threads per block, out[2] = blocks PER
 * FRAME, out[3] = lanes per environment: the batch's, doubled until a block fits 64 KB (at 64 lanes the taxels per trip halve instead).  They
 * depend on with_params and on nothing else of a call.  out = int32[4]. */
int tsim_tactile_normal_equations_launch_info(const tsim_batch* b, int with_params, int32_t* out);

/* sim.backward() results df_dq0 / df_dqdot0                    envs/redmax_torch_functions.py:92-100
 * = the carried adjoint once the whole tape has been popped. [B][ndof_r] each. */
int tsim_get_adjoint(tsim_batch* b, void* df_dq0, void* df_dqd0, void* stream);

/* sim.saveBackwardCache() / popBackwardCache() / clearBackwardCache()
 *                                     envs/redmax_torch_functions.py:65,81; envs/tactile_insertion_env.py:226
 * LIFO of tapes so that several episodes can be forwarded before their backwards.  The tapes are swapped by pointer:
 * save parks the live tape buffer on the stack and continues on a spare one (the current state is carried over), pop
 * makes the newest saved tape the live one again (its length and recording flag with it; the carried adjoint restarts at
 * zero) and returns the buffer it replaces to the pool.  No tape copy, no synchronisation; the only allocation is the first
 * use of a stack depth, which tsim_cache_reserve(depth) moves out of the hot path.  clear drops the saved tapes (their
 * buffers go back to the pool; two spares are kept).  All calls of one batch on ONE stream. */
int tsim_cache_save(tsim_batch* b, void* stream);
int tsim_cache_pop(tsim_batch* b, void* stream);
int tsim_cache_clear(tsim_batch* b);
int tsim_cache_reserve(tsim_batch* b, int depth);     /* no reference counterpart: pre-allocate `depth` tape buffers */
int tsim_cache_depth(const tsim_batch* b);            /* saved tapes on the stack */

/* Diagnostics (no reference counterpart): one residual evaluation g(q1; q0, qd0, u) and its Newton matrix
 * H = dg/dq1 for env 0..B-1; g_out [B][nr], H_out [B][nr][nr] (row-major). Used by the parity tests.
 * cycles (device int64 [B][32], may be NULL): shader-clock stamps taken inside the evaluation (models with ndof_r <= 8). */
int tsim_debug_eval(tsim_batch* b, const void* q1, const void* q0, const void* qd0, const void* u,
                    void* g_out, void* H_out, long long* cycles, void* stream);

/* Diagnostics (no reference counterpart; SURVEY.md §7 "Non-smoothness"): branch signature of the taped sub-steps
 * t_first+1 .. t_first+n (1 = the first sub-step after reset) of every environment: which contact points and taxels
 * penetrate and on which smooth piece of the penalty law each of them is (stick / slip, face of the primitive), recomputed
 * from the taped state exactly as the adjoint re-evaluates it.  out: DEVICE uint32 [n][B][2] = (number of penetrating
 * items, sum over them of mix(item, branch) mod 2^32; the oracle states the same two numbers).  Two runs with equal
 * signatures went through the same smooth pieces of the dynamics — the fp32 / fp64 gradient comparison is made on those
 * environments, and the fraction that differs is reported (tests/test_gpu_configs.py).  Needs reset(backward_flag=True). */
int tsim_debug_signature(tsim_batch* b, int t_first, int n, uint32_t* out, void* stream);

/* Diagnostics: the adjoint kernels of this batch record shader-clock stamps of the first sub-steps of wavefront 0 in `cycles`
 * (DEVICE int64[32], zero it first; NULL switches it off): loop top | tape record in LDS | phase 1 | output partials | solve |
 * contacts (3 stamps per pair group) | projection | mass product. */
int tsim_debug_stamps(tsim_batch* b, long long* cycles);

/* launch statistics of the most recent kernels (HIP events are the caller's business; this only reports
 * static launch geometry of the forward / backward kernels): out[0] = LDS bytes per block, out[1] = threads per block,
 * out[2] = blocks, out[3] = lanes per environment (64 / 32 / 16: a 64-lane block carries 1 / 2 / 4 environments; chosen
 * from the batch size and the device's SIMD count, override with the environment variable TSIM_LPE at
 * tsim_batch_create). out = int32[4]. */
int tsim_launch_info(const tsim_batch* b, int32_t* out);
/* Measurement (no reference counterpart; what bench.py's per-kernel roofline is timed with): while enabled, every launch of the simulation
 * kernels by this batch — k_forward, the tactile read-out kernel that follows it (k_taxels / k_taxels_small), k_backward — is bracketed by a
 * pair of HIP events recorded on the stream the kernel is launched on (never inside a stream capture).  tsim_kernel_times waits for the
 * recorded pairs, returns per kind the summed milliseconds and the number of launches since the previous call (HOST double[TSIM_KT_COUNT],
 * int32[TSIM_KT_COUNT]) and forgets them; at most 65 536 launches are kept between two calls (later ones are not timed). */
enum { TSIM_KT_FORWARD = 0, TSIM_KT_TAXELS = 1, TSIM_KT_BACKWARD = 2, TSIM_KT_COUNT = 3 };
int tsim_kernel_timing(tsim_batch* b, int enable);
int tsim_kernel_times(tsim_batch* b, double* ms_sum, int32_t* launches);
/* Force 16 / 32 / 64 lanes per environment (0 = automatic again).  For callers that split a batch into groups on several
 * streams: each group is then small, but the groups together should still fill the device. */
int tsim_set_lanes_per_env(tsim_batch* b, int lanes);   /* host-side only: takes effect with the next launch */
/* Statically known models.  The library carries, next to the generic kernels, instantiations of the forward / adjoint kernels for models
 * whose compiled blob it was built with (csrc/tsim_static.h; round 4: TactilePush, envs/assets/pusher/pusher.xml): tree, joint types, joint
 * frames and axes, contact pairs, dof records are compile-time constants there and the whole residual evaluation is one register-resident
 * pass (csrc/tsim_static_eval.h).  They are used when the
 * batch's blob equals the compiled-in one (checked at tsim_batch_create / tsim_update_model: ints and float records bit for bit — for an fp32
 * batch the records AS FLOATS, which is all its kernels ever see of them; round 5 added fp64 instantiations) and the batch has no
 * per-environment tables; results equal the generic kernels' to fp32 rounding (tests/test_gpu_static_model.py).
 * tsim_static_model returns the id of the instantiation the NEXT launch will use (0: generic, 1: TactilePush); tsim_set_static(b, 0)
 * keeps a batch on the generic kernels (also: environment variable TSIM_NO_STATIC at creation), tsim_set_static(b, 1) allows them again. */
int tsim_static_model(const tsim_batch* b);
int tsim_set_static(tsim_batch* b, int allow);
/* Name of the kernel instantiation the NEXT forward / adjoint launch of this batch uses, for measurement records (bench.py
 * `kernel_instantiation`): "generic", "static:<model>" (every float of the model a compile-time constant) or "param:<model>" (round 5: the
 * model's STRUCTURE — tree, joint types, contact pairs, which joint frames are identities and which axes unit vectors — is compiled in, its
 * parameters are read from the batch's float records, shared or per environment: the instantiation survives tsim_update_model and
 * tsim_set_env_tables as long as the structure does).  Returns a pointer into static storage. */
const char* tsim_kernel_variant(const tsim_batch* b);
/* Host-side switches of a batch (take effect with the next launch).  No reference counterpart.
 *   TSIM_OPT_PAIR_CULL  (default 1; environment variable TSIM_NO_PAIR_CULL=1 at creation: 0)  a contact pair whose points' bounding sphere is
 *                       out of reach of its primitive in every environment of a wavefront is skipped by the residual evaluation, and the
 *                       generic fp32 kernels test a point's fp32 distance before its double-precision one.  Exact: what is skipped would
 *                       have contributed zeros (tests/test_gpu_exact_options.py asserts equal outputs with the option off). */
/*   TSIM_OPT_VALUE_TRIALS (default 2; environment variable TSIM_VALUE_TRIALS=n at creation; 0: off)  a line-search trial only needs ||g||: after
 *                       this many rejected trials of a Newton iteration the further ones evaluate the residual WITHOUT its tangents (about half
 *                       the work) whenever no environment of the wavefront needs a Newton matrix from that round; a trial that is taken is
 *                       re-evaluated in full first.  Exact: iterates, convergence flags and the taped matrices are those of the loop without
 *                       the option (tests/test_gpu_exact_options.py); tsim_last_evals counts trial points either way. */
/*   TSIM_OPT_TRIAL_HELPERS (default 1; environment variable TSIM_NO_TRIAL_HELPERS=1 at creation: 0)  a launch lasts as long as its slowest
 *                       environment's chain of evaluations, and those chains are long line searches.  The slots of a wavefront whose own
 *                       environments are finished evaluate the NEXT trial points (dlbase + 2^-t dq: known in advance) of a slot that is still
 *                       in a line search; the owner judges the results in the order and with the decision code of the sequential loop.
 *                       Exact: iterates, convergence flags, taped matrices and tsim_last_evals are those of the loop without helpers
 *                       (tests/test_gpu_exact_options.py); a line search of n trials takes ceil(n / (1 + helpers)) rounds. */
/*   TSIM_OPT_VALUE_FIRST (default 1; environment variable TSIM_NO_VALUE_FIRST=1 at creation: 0)  launches that record no tape (roll-out collection:
 *                       tsim_reset with backward_flag 0) never use the Newton matrix of a sub-step's FINAL iterate.  Where the previous sub-step
 *                       of an environment converged in one Newton step, the first trial of the next one evaluates the residual without its
 *                       tangents; it is taken as it is if it ends the sub-step, and evaluated again in full otherwise.  Exact, as above. */
/* Read-only through tsim_get_option (set them with tsim_set_solver_options): TSIM_OPT_CROSS_KINKS, TSIM_OPT_EVAL_BUDGET; and TSIM_OPT_ALL_DEFAULT = 1 iff
 * every solver / scheduling option of the batch is at its default (cross_kinks 1, eval_budget 0, value_trials 2, trial_helpers 1, value_first 1) — the
 * forward launch of an fp32 batch on a compiled-in model at four environments per wavefront then runs an instantiation that has them as compile-time
 * constants (same results bit for bit, ~2 % faster; environment variable TSIM_NO_DEFAULT_OPTS=1 at creation: never).
 * TSIM_OPT_FRAME_RECORDS (read-only): how the newest forward launch wrote its frames' q / qd / variables / pose records.  0: inside the forward kernel, at
 * the end of each frame; 1: after it, from the tape, by the frame-record pass — tsim_rollout launches of more than one frame on a fused compiled-in
 * model that record a tape and read the tactile frames out after the launch; 2: ... and the forward kernel was the instantiation that has this as a
 * compile-time constant (every option at its default).  The same results bit for bit (tests/test_gpu_frame_records.py); environment variable
 * TSIM_INKERNEL_FRAME_OUT=1 at creation: always 0.
 * TSIM_OPT_FORWARD_SPLIT (read-only): 1 iff the newest forward launch went out as two — the heaviest eighth of its wavefronts (by the order the
 * previous episode launch of the same length left) on the caller's stream, the others with their read-out on a side stream of the batch, which the
 * caller's stream waits for before the call returns: the light environments' frames are read out while the heavy ones are still being simulated.
 * Launches with TSIM_OPT_FRAME_RECORDS != 0 that have that order, a batch that is a multiple of the environments per wavefront, 64 blocks or more and
 * no more than the device holds at once; never inside a stream capture.  The same results bit for bit (tests/test_gpu_forward_split.py);
 * environment variable TSIM_NO_FORWARD_SPLIT=1 at creation: always 0.
 * TSIM_OPT_PREDICTOR_HELPERS (default 1; environment variable TSIM_NO_PREDICTOR_HELPERS=1 at creation: 0; nothing without TSIM_OPT_TRIAL_HELPERS)  most
 * sub-steps are two rounds, the evaluation at the predictor and the one at the trial point that is committed, and the next sub-step's predictor follows
 * from that trial point alone.  A slot whose own environment is finished evaluates it in the same round; if the trial is committed, its environment
 * starts the next sub-step from that evaluation: one round per sub-step while a finished slot shares the wavefront.  Fused compiled-in BDF1 models,
 * free-running launches that record a tape.  Exact, as TSIM_OPT_TRIAL_HELPERS is (tests/test_gpu_predictor_helpers.py); tsim_last_helper_trials also
 * counts the predictors taken over.  It is no part of TSIM_OPT_ALL_DEFAULT: the instantiations read it at run time.
 * TSIM_OPT_ADJOINT_PREPASS (set: 0 | 1, default 1; environment variable TSIM_NO_ADJOINT_PREPASS=1 at creation: 0)  tsim_backward_episode of a fused
 * compiled-in model (fp32, 16 lanes per environment, BDF1, no parameter gradient set) computes the frames' seed partials — (dvar/dq)^T w_var +
 * (dtac/dq)^T w_tac and (dtac/dqd)^T w_tac at each frame's taped final state — in a pass of its own over (frame, environment) items,
 * k_adjoint_seeds, and the adjoint kernel (k_backward_pre) adds them instead of evaluating the tactile law inside its serial chain.  Same stream,
 * same results bit for bit (tests/test_gpu_adjoint_prepass.py); the pass's buffer, tape capacity x B x 2 ndof_r reals, is allocated with the
 * batch (if that fails the batch keeps the in-kernel path).  tsim_get_option reads whether the most recent adjoint launch took the path.  It is no
 * part of TSIM_OPT_ALL_DEFAULT. */
enum { TSIM_OPT_PAIR_CULL = 1, TSIM_OPT_VALUE_TRIALS = 2, TSIM_OPT_TRIAL_HELPERS = 3, TSIM_OPT_VALUE_FIRST = 4, TSIM_OPT_CROSS_KINKS = 5, TSIM_OPT_EVAL_BUDGET = 6,
       TSIM_OPT_ALL_DEFAULT = 7, TSIM_OPT_FRAME_RECORDS = 8, TSIM_OPT_FORWARD_SPLIT = 9, TSIM_OPT_PREDICTOR_HELPERS = 10, TSIM_OPT_ADJOINT_PREPASS = 11 };
int tsim_set_option(tsim_batch* b, int option, int value);
int tsim_get_option(const tsim_batch* b, int option);

/* residual evaluations each environment spent in the most recent tsim_step (HOST int32[B]); synchronises. */
int tsim_last_evals(tsim_batch* b, int32_t* host_out);
/* ... and how many of those trial points were evaluated by a helper slot (TSIM_OPT_TRIAL_HELPERS) instead of in a round of the environment's own
 * (HOST int32[B]); synchronises.  No reference counterpart (diagnostics: tests assert that the helper path ran, profiles report its share). */
int tsim_last_helper_trials(tsim_batch* b, int32_t* host_out);

/* The Newton iteration of a sub-step is the loop the model's <solver_option tol max_iter max_ls> states (envs/assets/pusher/pusher.xml:4)
 * and nothing else: up to max_iter iterations, each halving its step until ||g|| decreases, at most max_ls times, taking the last trial
 * if none did; converged when ||g||_2 < tol.  fp64 batches run exactly that by default.  Two options around it, neither of which the
 * reference has (its arithmetic is fp64 and it runs one environment at a time):
 *   cross_kinks  (default: 1 for TSIM_F32, 0 for TSIM_F64)  a line search whose max_ls + 1 trials all fail is a non-smooth local minimum
 *                of ||g|| at a contact / friction kink.  The literal loop gets across it with its 2^-max_ls step and ~150 more
 *                evaluations in fp64; in fp32 it often does not (step lengths of 1e-6 drown in rounding) and runs to max_iter while the
 *                rest of the batch waits.  With the option, and only when ||g|| < TSIM_KINK_FACTOR x tol (close to convergence, where the
 *                Newton step is small), a trial still rejected after TSIM_KINK_LS halvings is followed by the full Newton step across
 *                the kink, at most TSIM_KINK_MAX times per sub-step: the same root, ~20 evaluations.  Everywhere else the loop is the
 *                literal one.
 *   eval_budget  (default 0 = none)  residual evaluations one sub-step may take; a sub-step cut short is flagged in status exactly like
 *                one that hit max_iter.  For throughput-minded roll-out collection on stiff models (a TactileInsertion grasp can make
 *                plain backtracking creep for ~2000 evaluations, and a batch waits for its slowest environment).
 * Host-side only: takes effect with the next launch. */
#define TSIM_KINK_FACTOR 1000.0
#define TSIM_KINK_LS 4
#define TSIM_KINK_MAX 6
int tsim_set_solver_options(tsim_batch* b, int cross_kinks, int eval_budget);
/* largest ||g||_2 any sub-step of the most recent forward launch ended with, per environment (HOST float[B]); synchronises. */
int tsim_last_gnorm(tsim_batch* b, float* host_out);

const char* tsim_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
