"""Autograd surface of the hot path.

* `StepSimFunction`, `EpisodicSimFunction` — same names, argument order, outputs and simulator call protocol as the
  reference's envs/redmax_torch_functions.py:11-174 (one environment, a `redmax_py.Simulation`-like object; numpy
  float64 across the binding).  The reference's own file also runs unmodified on top of compat/redmax_py.py; these
  re-statements exist so that the package is usable without the reference checkout and so that the call protocol is
  pinned by tests/test_protocol.py against a trace recorded from the reference's functions.
* `BatchedStepSimFunction` — the MI355X-native counterpart: B environments per call, tensors stay on the device, one
  forward kernel launch per env-step and one adjoint launch per env-step (tactilesimulation_amd.host.BatchSim).
* `BatchedEpisodicSimFunction` — batched counterpart of EpisodicSimFunction: the whole open-loop episode of B
  environments in ONE forward launch and ONE adjoint launch (tsim_rollout / tsim_backward_episode).
* `BatchedEpisodicParamSimFunction` — the same episode with the per-environment numeric tables as one more differentiable
  input (the reference's flag_p / df_dp, batched, for contact, tactile and damping parameters: include/tsim.h tsim_set_param_grad).
"""
import numpy as np
import torch
from torch import autograd


def _to_torch(x, dtype, device, requires_grad):
    return torch.tensor(x, dtype=dtype, device=device, requires_grad=requires_grad)


class StepSimFunction(autograd.Function):
    """(action[ndof_u], num_steps, sim, grad_mode) -> q[ndof_r], var[ndof_var], tactile[ndof_tactile]
    Holds `action` for num_steps sub-steps and returns the last frame.  State-to-state gradient flow lives inside the
    simulator (tape + carried adjoint); only `action` is a differentiable input."""

    @staticmethod
    def forward(ctx, action, num_steps, sim, grad_mode):
        ctx.sim, ctx.num_steps = sim, num_steps
        ctx.need_du = action.requires_grad
        ctx.device, ctx.dtype = action.device, action.dtype
        sim.set_u(action.detach().cpu().numpy())
        sim.forward(num_steps, verbose=False, test_derivatives=False, save_last_frame_var_only=True)
        q = _to_torch(sim.get_q().copy(), ctx.dtype, ctx.device, grad_mode)
        var = _to_torch(sim.get_variables().copy(), ctx.dtype, ctx.device, grad_mode)
        tactile = _to_torch(sim.get_tactile_force_vector(), ctx.dtype, ctx.device, grad_mode)
        return q, var, tactile

    @staticmethod
    def backward(ctx, df_dq, df_dvar, df_dtactile):
        sim, n = ctx.sim, ctx.num_steps
        sim.backward_info.set_flags(flag_q0=False, flag_qdot0=False, flag_p=False, flag_u=ctx.need_du)

        def last_block(g, dim):          # partials are w.r.t. the LAST of the n sub-steps; earlier blocks are zero
            full = np.zeros(dim * n)
            if dim:
                full[-dim:] = g.reshape(-1).detach().cpu().numpy()
            return full
        sim.backward_info.df_dq = last_block(df_dq, sim.ndof_r)
        sim.backward_info.df_dvar = last_block(df_dvar, sim.ndof_var)
        sim.backward_info.df_dtactile = last_block(df_dtactile, sim.ndof_tactile)
        sim.backward_info.df_du = np.zeros(sim.ndof_u * n)
        sim.backward_steps(n)
        if not ctx.need_du:
            return None, None, None, None
        du = sim.backward_results.df_du.copy().reshape(n, sim.ndof_u)    # autograd sum-reduces (n, nu) -> (nu,)
        return _to_torch(du, ctx.dtype, ctx.device, True), None, None, None


class EpisodicSimFunction(autograd.Function):
    """(q0, qdot0, actions[T, ndof_u], tactile_masks[T] bool, sim, grad_mode) -> qs[T, ndof_r], vars[T, ndof_var],
    tactiles[sum(mask), ndof_tactile].  One sub-step per action."""

    @staticmethod
    def forward(ctx, q0, qdot0, actions, tactile_masks, sim, grad_mode):
        T = actions.shape[0]
        ctx.sim, ctx.T = sim, T
        ctx.need_q0, ctx.need_qdot0, ctx.need_du = q0.requires_grad, qdot0.requires_grad, actions.requires_grad
        ctx.device, ctx.dtype = q0.device, q0.dtype
        ctx.tactile_masks = tactile_masks
        a_np = actions.detach().cpu().numpy()
        sim.set_state_init(q0.detach().cpu().numpy(), qdot0.detach().cpu().numpy())
        sim.reset(backward_flag=grad_mode)
        qs, vs, ts = [], [], []
        for t in range(T):
            sim.set_u(a_np[t])
            sim.forward(1, verbose=False, test_derivatives=False)
            qs.append(_to_torch(sim.get_q().copy(), ctx.dtype, ctx.device, grad_mode))
            vs.append(_to_torch(sim.get_variables().copy(), ctx.dtype, ctx.device, grad_mode))
            if tactile_masks[t]:
                ts.append(_to_torch(sim.get_tactile_force_vector().copy(), ctx.dtype, ctx.device, grad_mode))
        if grad_mode:
            sim.saveBackwardCache()
        return torch.stack(qs, dim=0), torch.stack(vs, dim=0), torch.stack(ts, dim=0)

    @staticmethod
    def backward(ctx, df_dq, df_dvar, df_dtactile):
        sim, T = ctx.sim, ctx.T
        sim.popBackwardCache()
        sim.backward_info.set_flags(flag_q0=ctx.need_q0, flag_qdot0=ctx.need_qdot0, flag_p=False, flag_u=ctx.need_du)
        sim.backward_info.df_dq = df_dq.reshape(-1).detach().cpu().numpy()
        sim.backward_info.df_dvar = df_dvar.reshape(-1).detach().cpu().numpy()
        # As the reference does (envs/redmax_torch_functions.py:87): only the frames the mask selected, sum(mask) x ndof_tactile values.
        # The simulator knows which sub-steps had their tactile frame read (compat/redmax_py.py records every get_tactile_force_vector()
        # after a forward) and puts each block on its sub-step.
        sim.backward_info.df_dtactile = df_dtactile.reshape(-1).detach().cpu().numpy()
        sim.backward_info.df_dq0 = np.zeros(sim.ndof_r)
        sim.backward_info.df_dqdot0 = np.zeros(sim.ndof_r)
        sim.backward_info.df_du = np.zeros(sim.ndof_u * T)
        sim.backward()
        res = sim.backward_results
        g_q0 = _to_torch(res.df_dq0.copy(), ctx.dtype, ctx.device, True) if ctx.need_q0 else None
        g_qd0 = _to_torch(res.df_dqdot0.copy(), ctx.dtype, ctx.device, True) if ctx.need_qdot0 else None
        g_u = _to_torch(res.df_du.copy().reshape(T, sim.ndof_u), ctx.dtype, ctx.device, True) if ctx.need_du else None
        return g_q0, g_qd0, g_u, None, None, None


class BatchedStepSimFunction(autograd.Function):
    """(action[B, ndof_u], num_steps, batch_sim, grad_mode) -> q[B, ndof_r], var[B, ndof_var], tactile[B, ndof_tactile]

    Batched, device-resident counterpart of StepSimFunction: no numpy hop, one HIP launch forward and one backward per
    env-step for all B environments.  As in the reference, outputs are fresh leaves of the autograd graph (the
    state-to-state chain is carried inside the simulator), so backward calls must arrive newest-first — which autograd
    guarantees whenever action_{t+1} depends on the outputs of step t, and which callers of open-loop roll-outs get by
    summing a loss over steps in order."""

    @staticmethod
    def forward(ctx, action, num_steps, sim, grad_mode):
        ctx.sim, ctx.num_steps = sim, num_steps
        ctx.need_du = action.requires_grad
        ctx.in_dtype = action.dtype
        out = sim.step(action.detach(), num_steps)
        q, var, tac = out["q"], out.get("var"), out.get("tactile")
        if var is None:
            var = q.new_zeros((sim.B, 0))
        if tac is None:
            tac = q.new_zeros((sim.B, 0))
        ctx.status = out["status"]
        res = tuple(t.to(action.dtype) for t in (q, var, tac))
        if not grad_mode:
            ctx.mark_non_differentiable(*res)
        return res

    @staticmethod
    def backward(ctx, df_dq, df_dvar, df_dtactile):
        sim, n = ctx.sim, ctx.num_steps
        # one frame of n sub-steps: the kernel sums df_du over the frame's sub-steps itself (include/tsim.h tsim_backward_episode)
        f = lambda t, on: t.to(sim.dtype).unsqueeze(0) if (on and t is not None) else None
        du = sim.backward_episode(1, n, f(df_dq, True), f(df_dvar, sim.ndof_var), f(df_dtactile, sim.ndof_tactile))
        if not ctx.need_du:
            return None, None, None, None
        return du[0].to(ctx.in_dtype), None, None, None


class BatchedEpisodicSimFunction(autograd.Function):
    """(q0[B, ndof_r], qdot0[B, ndof_r], actions[T, B, ndof_u], tactile_masks bool[T], batch_sim, grad_mode, num_steps=1)
        -> qs[T, B, ndof_r], vars[T, B, ndof_var], tactiles[sum(mask), B, ndof_tactile]

    Batched, device-resident counterpart of EpisodicSimFunction (envs/redmax_torch_functions.py:11-109): same argument
    order and meaning with a batch axis after the time axis, the reference's `forward(1)` per action generalised to
    `num_steps` sub-steps per action.  Like the reference it saves the tape on the backward cache in forward and pops it
    in backward, so several episodes may be forwarded before their backward passes (newest first)."""

    @staticmethod
    def forward(ctx, q0, qdot0, actions, tactile_masks, sim, grad_mode, num_steps=1):
        ctx.sim, ctx.T, ctx.num_steps = sim, int(actions.shape[0]), int(num_steps)
        ctx.need = (q0.requires_grad, qdot0.requires_grad, actions.requires_grad)
        ctx.in_dtype = actions.dtype
        ctx.tactile_masks = tactile_masks
        sim.reset(q0.detach(), qdot0.detach(), backward_flag=grad_mode)
        out = sim.rollout(actions.detach(), ctx.num_steps, tactile_mask=tactile_masks)
        qs, vars_, tacs = out["q"], out.get("var"), out.get("tactile")
        if vars_ is None:
            vars_ = qs.new_zeros((ctx.T, sim.B, 0))
        if tacs is None:
            tacs = qs.new_zeros((0, sim.B, 0))
        ctx.status = out["status"]
        if grad_mode:
            sim.cache_save()
        res = tuple(t.to(actions.dtype) for t in (qs, vars_, tacs))
        if not grad_mode:
            ctx.mark_non_differentiable(*res)
        return res

    @staticmethod
    def backward(ctx, df_dq, df_dvar, df_dtactile):
        sim = ctx.sim
        sim.cache_pop()
        du = sim.backward_episode(ctx.T, ctx.num_steps, df_dq, df_dvar if sim.ndof_var else None,
                                  df_dtactile if (sim.ndof_tactile and df_dtactile.shape[0] > 0) else None,
                                  tactile_mask=ctx.tactile_masks)
        lq, lv = sim.get_adjoint()
        g = (lq.to(ctx.in_dtype) if ctx.need[0] else None, lv.to(ctx.in_dtype) if ctx.need[1] else None,
             du.to(ctx.in_dtype) if ctx.need[2] else None)
        return g + (None, None, None, None)


class BatchedEpisodicParamSimFunction(autograd.Function):
    """(q0[B, ndof_r], qdot0[B, ndof_r], actions[T, B, ndof_u], tables[B, table_size], tactile_masks bool[T], batch_sim, grad_mode, num_steps=1)
        -> qs[T, B, ndof_r], vars[T, B, ndof_var], tactiles[sum(mask), B, ndof_tactile]

    BatchedEpisodicSimFunction with the environments' numeric tables (BatchSim.set_env_tables: one row per environment, the model's F[] layout)
    as an input: forward sets them and runs the episode, backward returns next to the q0 / qdot0 / action gradients (the same numbers as
    BatchedEpisodicSimFunction's) the gradient w.r.t. the tables.  It is non-zero only at model.param_columns() — contact pair and tactile
    sensor kn kt mu damping, dof damping — and, once batch_sim.set_param_grad_groups switched them on, at model.body_param_columns(): link
    mass / centre of mass / inertia, motor lo hi P D, dof limits.  Geometry and the rest of a row are not differentiated.  A shared parameter is
    `base.expand(B, -1)`: autograd sums the rows.  The tables stay set on the batch after forward (its backward needs them)."""

    @staticmethod
    def forward(ctx, q0, qdot0, actions, tables, tactile_masks, sim, grad_mode, num_steps=1):
        ctx.sim, ctx.T, ctx.num_steps = sim, int(actions.shape[0]), int(num_steps)
        ctx.need = (q0.requires_grad, qdot0.requires_grad, actions.requires_grad, tables.requires_grad)
        ctx.in_dtype, ctx.tab_dtype = actions.dtype, tables.dtype
        ctx.tactile_masks = tactile_masks
        ctx.tables = tables.detach().to(device=sim.device, dtype=sim.dtype).contiguous()
        sim.set_env_tables(ctx.tables)
        sim.reset(q0.detach(), qdot0.detach(), backward_flag=grad_mode)
        out = sim.rollout(actions.detach(), ctx.num_steps, tactile_mask=tactile_masks)
        qs, vars_, tacs = out["q"], out.get("var"), out.get("tactile")
        if vars_ is None:
            vars_ = qs.new_zeros((ctx.T, sim.B, 0))
        if tacs is None:
            tacs = qs.new_zeros((0, sim.B, 0))
        ctx.status = out["status"]
        if grad_mode:
            sim.cache_save()
        res = tuple(t.to(actions.dtype) for t in (qs, vars_, tacs))
        if not grad_mode:
            ctx.mark_non_differentiable(*res)
        return res

    @staticmethod
    def backward(ctx, df_dq, df_dvar, df_dtactile):
        sim = ctx.sim
        sim.cache_pop()
        if getattr(sim, "_env_tables", None) is not ctx.tables:      # another episode set its own tables since: the adjoint needs this one's
            sim.set_env_tables(ctx.tables)
        gtab = None
        if ctx.need[3]:
            gtab = torch.zeros_like(ctx.tables)
            sim.set_param_grad(gtab)
        try:
            du = sim.backward_episode(ctx.T, ctx.num_steps, df_dq, df_dvar if sim.ndof_var else None,
                                      df_dtactile if (sim.ndof_tactile and df_dtactile.shape[0] > 0) else None,
                                      tactile_mask=ctx.tactile_masks)
        finally:
            if gtab is not None:
                sim.set_param_grad(None)
        lq, lv = sim.get_adjoint()
        g = (lq.to(ctx.in_dtype) if ctx.need[0] else None, lv.to(ctx.in_dtype) if ctx.need[1] else None,
             du.to(ctx.in_dtype) if ctx.need[2] else None, gtab.to(ctx.tab_dtype) if gtab is not None else None)
        return g + (None, None, None, None)


def episode_jacobian(sim, num_frames, num_steps, columns, tactile_mask=None, outputs=("q", "var", "tactile")):
    """Jacobian of the frames' outputs of the recorded episode w.r.t. table columns, per environment — the forward-mode companion of
    BatchedEpisodicParamSimFunction's table gradient (which gives one row J^T w per backward pass; this gives J column by column).

    sim holds the tape of the newest num_frames x num_steps sub-steps (reset(backward_flag=True) + rollout, e.g. the forward of
    BatchedEpisodicParamSimFunction with grad_mode); columns: entries of sim.model.param_columns() or sim.model.body_param_columns() — (kind,
    name, field, column) — or plain column indices: the contact columns, and those body columns whose group ('inertial': link mass, centre of
    mass, inertia; 'motor': lo hi P D; 'limit': lo hi k) is on in sim.param_grad_groups() — BatchSim.tangent_episode reads no other, so a body
    column whose group is off is refused rather than answered with zeros.  One unit direction per column, eight per launch
    (include/tsim.h tsim_tangent_episode); the tape, the state and the carried adjoint are left as they are, so the episode's backward pass may
    follow.  Returns [B, n_out, len(columns)] with n_out the outputs named in `outputs`, each flattened frame-major ([T, dim], tactile:
    [n_masked, dim]) and concatenated in the order q, var, tactile."""
    cols = [int(c[3]) if isinstance(c, (tuple, list)) else int(c) for c in columns]
    allowed = {int(c) for (_, _, _, c) in sim.model.param_columns()}
    group_of = {int(c): {"link": "inertial"}.get(kind, kind) for (kind, _, _, c) in sim.model.body_param_columns()}
    on = set(sim.param_grad_groups())
    bad = [c for c in cols if c not in allowed and c not in group_of]
    if bad:
        raise ValueError("episode_jacobian: columns %s are not among model.param_columns() or model.body_param_columns()" % bad)
    off = sorted({group_of[c] for c in cols if c in group_of and group_of[c] not in on})
    if off:
        raise ValueError("episode_jacobian: columns %s belong to the body group(s) %s, which the tangent pass reads only once they are on: "
                         "sim.set_param_grad_groups(%r)" % ([c for c in cols if group_of.get(c) in off], off, tuple(sorted(on | set(off)))))
    ntab = sim.base_tables().shape[1]
    keys = [k for k in ("q", "var", "tactile") if k in outputs and (k == "q" or getattr(sim, "ndof_" + k))]
    blocks = []
    for c0 in range(0, len(cols), sim.TANGENT_MAX_DIR):
        chunk = cols[c0:c0 + sim.TANGENT_MAX_DIR]
        dt = torch.zeros((len(chunk), sim.B, ntab), device=sim.device, dtype=sim.dtype)
        for d, c in enumerate(chunk):
            dt[d, :, c] = 1.0
        o = sim.tangent_episode(num_frames, num_steps, dtables=dt, tactile_mask=tactile_mask, want_var="var" in keys, want_tactile="tactile" in keys)
        # [ndir, n, B, dim] -> [B, n * dim, ndir]
        blocks.append(torch.cat([o["d" + k].permute(2, 1, 3, 0).reshape(sim.B, -1, len(chunk)) for k in keys], 1))
    if not blocks:
        return torch.zeros((sim.B, 0, 0), device=sim.device, dtype=sim.dtype)
    return torch.cat(blocks, 2)


def episode_transition(sim, num_frames, num_steps):
    """Local linearisation of the recorded episode's dynamics, per environment and env-step: (A, B) with A [T, B, 2 nr, 2 nr] and
    B [T, B, 2 nr, nu], T = num_frames, x = (q, qd):

        x_{f+1} = A_f x_f + B_f u_f          (to first order around the recorded roll-out; u_f held for the frame's num_steps sub-steps)

    so  dx_T = A_{T-1} ... A_0 dx_0 + sum_f A_{T-1} ... A_{f+1} B_f du_f  — the q-rows of these products are what BatchSim.tangent_episode returns
    as dq for the direction (dx_0, du), and what episode_jacobian gives column by column for TABLE columns; episode_jacobian differentiates the
    frames' outputs w.r.t. parameters over the whole episode, this differentiates one frame's end state w.r.t. that frame's start state and
    control.  What iLQR / DDP, a time-varying LQR or an EKF around a recorded push take; the product of the A_f's spectral norms bounds the growth
    of a BPTT gradient through the episode.

    sim holds the tape of the newest num_frames x num_steps sub-steps (reset(backward_flag=True) + rollout).  One launch for every frame
    (include/tsim.h tsim_frame_jacobians); the tape, the state and the carried adjoint are left as they are, so the episode's backward pass may
    follow.  BDF1 models only."""
    o = sim.frame_jacobians(num_frames, num_steps, want_A=True, want_B=True, want_var=False)
    return o["A"], o["B"]


def episode_observation(sim, num_frames, num_steps, tactile_mask=None):
    """The measurement map that goes with episode_transition: C [n_masked, B, ndof_tactile, 2 nr], C_f = dtactile / dx at the END state of masked
    frame f, x = (q, qd) taken as independent variables — the tactile frame is what this simulator measures.  With (A, B) of episode_transition,
    around the recorded roll-out and to first order:

        dx_{f+1} = A_f dx_f + B_f du_f ,      dtac_f = C_f dx_{f+1}          (so C_f A_f, C_f B_f: the response to the frame's start state and control)

    which is what a linearised (extended) Kalman filter around a recorded push takes: predict  x^- = A_f x^ + B_f du_f,  P^- = A_f P A_f^T + Q;
    update with the innovation  y_f - C_f x^-  (y_f: measured minus recorded tactile frame); in information form  P^-1 = (P^-)^-1 + C_f^T R^-1 C_f,
    P^-1 x^ = (P^-)^-1 x^- + C_f^T R^-1 y_f, with C_f^T R^-1 C_f only 2 nr x 2 nr.  An unloaded taxel's row is exactly zero; at a stick / slip
    switch the row is the one-sided derivative of the piece the taxel is on.

    The result is the transposed VIEW (no copy) of BatchSim.tactile_jacobians' Ct [n_masked, B, 2 nr, ndof_tactile], whose rows are contiguous
    tactile frames: C.transpose(-1, -2) is contiguous, C is not.  Size: 2 nr * ndof_tactile reals per environment and masked frame — TactilePush
    fp32 21 840 bytes (20 frames x 4096 environments: 1.79 GB), D'Claw 217 440 bytes (20 x 2048: 8.9 GB): mask the frames that are needed.

    sim holds the tape of the newest num_frames x num_steps sub-steps.  One launch for every masked frame (include/tsim.h tsim_tactile_jacobians);
    the tape, the state and the carried adjoint are left as they are.  BDF2 and rotation-vector models are accepted."""
    return sim.tactile_jacobians(num_frames, num_steps, tactile_mask).transpose(-1, -2)


def episode_parameters(sim, num_frames, num_steps, cols, tactile_mask=None):
    """The parameter block that completes episode_transition and episode_observation: (E, F) with E [T, B, 2 nr, ncols] and F [n_masked, B,
    ndof_tactile, ncols], p the table columns `cols` (out of model.param_columns(): per contact pair and per tactile sensor kn kt mu damping, per
    dof its damping), around the recorded roll-out and to first order:

        dx_{f+1} = A_f dx_f + B_f du_f + E_f dp ,      dtac_f = C_f dx_{f+1} + F_f dp

    E_f = dx_{f+1} / dp at fixed (x_f, u_f), F_f = dtactile / dp at fixed x_{f+1}.  What a joint state-and-parameter filter takes (augmented
    state (x, p): [[A, E], [0, I]], [C | F]), and multiple-shooting or equation-error identification, where every frame's residual Jacobian
    stands alone.  A sensor column is exactly zero in E (sensors do not enter the dynamics); F is non-zero only in a sensor column, and there only
    on that sensor's taxels: it is scattered from BatchSim.param_jacobians' compact Ft.  F is None for a model without taxels.

    sim holds the tape of the newest num_frames x num_steps sub-steps.  One launch per 32 columns (include/tsim.h tsim_param_jacobians); the tape,
    the state and the carried adjoint are left as they are.  BDF1 models only."""
    from .model import blob as B
    cols = [int(c) for c in cols]
    m, nmax = sim.model, sim.PARAM_JACOBIAN_MAX_COLS
    want_F = sim.ndof_tactile > 0
    E, Ft = [], None
    for c0 in range(0, len(cols), nmax):
        o = sim.param_jacobians(num_frames, num_steps, cols[c0:c0 + nmax], want_E=True, want_tactile=want_F and c0 == 0, tactile_mask=tactile_mask)
        E.append(o["E"])
        Ft = o.get("Ft", Ft)
    E = torch.cat(E, -1) if E else torch.zeros((int(num_frames), sim.B, 2 * sim.ndof_r, 0), device=sim.device, dtype=sim.dtype)
    if not want_F:
        return E, None
    if Ft is None:
        Ft = sim.param_jacobians(num_frames, num_steps, (), want_E=False, want_tactile=True, tactile_mask=tactile_mask)["Ft"]
    F = torch.zeros((Ft.shape[0], sim.B, sim.ndof_tactile, len(cols)), device=sim.device, dtype=sim.dtype)
    at = {c: k for k, c in enumerate(cols)}
    off, foff = int(m.I[B.TSIM_IH_OFF_SENSOR]), int(m.I[B.TSIM_IH_FOFF_SENSOR])
    for s in range(int(m.I[B.TSIM_IH_NSENSOR])):
        tx0, nt = (int(m.I[off + s * B.TSIM_SI_SIZE + i]) for i in (B.TSIM_SI_TAX0, B.TSIM_SI_NTAX))
        for f in range(4):      # kn kt mu damping: Ft's rows
            k = at.get(foff + s * B.TSIM_SF_SIZE + B.TSIM_SF_KN + f)
            if k is not None:
                F[:, :, 3 * tx0:3 * (tx0 + nt), k] = Ft[:, :, f, 3 * tx0:3 * (tx0 + nt)]
    return E, F


def episode_information(sim, num_frames, num_steps, weight=None, residual=None, cols=None, tactile_mask=None):
    """The tactile block of episode_observation / episode_parameters in information form: (N, n) with N [n_masked, B, Z, Z] = H_f^T W H_f and
    n [n_masked, B, Z] = H_f^T W r_f (None without `residual`), H_f = [C_f | F_f[:, cols]], Z = 2 nr + len(cols), over the augmented state
    (x, p[cols]) in the caller's column order — the layout of episode_parameters' E and F, so that a joint filter on [[A, E], [0, I]] takes it
    as it is.  `cols` are table columns out of model.param_columns() (None: the state block alone).  W = diag(weight) [ndof_tactile], an
    inverse variance per tactile value (None: ones); residual [n_masked, B, ndof_tactile].  The information-form measurement update is

        info = (P^-)^-1 + N_f ,      eta = (P^-)^-1 z^- + n_f          (r_f = y_f: measured minus predicted tactile frame, W = R^-1)

    and Gauss-Newton / LM on tactile residuals sums N_f and n_f over the frames.  A sensor's columns are gathered from the kernel's 4 nsensor
    parameter block; pair and dof-damping columns have no direct tactile term: their rows and columns are exact zeros.  N is exactly symmetric.

    Neither C_f nor F_f is stored: Z^2 + Z reals per environment and masked frame instead of (2 nr + 4) ndof_tactile — TactilePush with the
    sensor's four columns, fp32: 1 368 bytes instead of 27 300 (20 frames x 4096 environments: 0.11 GB instead of 2.2 GB); D'Claw at 2048
    environments x 20 frames: 0.17 GB instead of 8.9 GB + F.

    sim holds the tape of the newest num_frames x num_steps sub-steps.  One launch (include/tsim.h tsim_tactile_normal_equations); the tape, the
    state and the carried adjoint are left as they are.  BDF2 and rotation-vector models are accepted."""
    from .model import blob as B
    cols = [int(c) for c in cols] if cols is not None else []
    o = sim.tactile_normal_equations(num_frames, num_steps, weight=weight, residual=residual, with_params=bool(cols), tactile_mask=tactile_mask)
    N, n = o["N"], o.get("n")
    if not cols:
        return N, n
    m, xs = sim.model, 2 * sim.ndof_r
    foff = int(m.I[B.TSIM_IH_FOFF_SENSOR])
    src = {foff + s * B.TSIM_SF_SIZE + B.TSIM_SF_KN + f: xs + 4 * s + f for s in range(int(m.I[B.TSIM_IH_NSENSOR])) for f in range(4)}
    known = set(int(c[3]) for c in m.param_columns())
    for c in cols:
        if c not in known:
            raise ValueError("episode_information: table column %d is not a contact-group parameter (model.param_columns())" % c)
    # gather: the state, then per caller column its kernel column, or a zero one (the last, appended) for a pair or dof-damping column
    Zk = N.shape[-1]
    idx = torch.tensor(list(range(xs)) + [src.get(c, Zk) for c in cols], device=N.device)
    Np = torch.nn.functional.pad(N, (0, 1, 0, 1))
    N2 = Np.index_select(-2, idx).index_select(-1, idx)
    n2 = torch.nn.functional.pad(n, (0, 1)).index_select(-1, idx) if n is not None else None
    return N2, n2
