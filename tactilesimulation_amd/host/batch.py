"""BatchSim — B environments of one model resident on one MI355X, driven through the C ABI (include/tsim.h).

Device memory, streams and dtype plumbing come from PyTorch-ROCm; all simulation arithmetic runs in the
hand-written HIP kernels (tactilesimulation_amd/csrc). Host-side mirror of the stepping/adjoint part of the
reference's `redmax_py.Simulation`, batched.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from ..model import blob as _blob
from ..model.compiler import CompiledModel, load_model


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class BatchSim:
    def __init__(self, model, batch_size, device="cuda:0", dtype=torch.float32, tape_capacity=512):
        if isinstance(model, str):
            model = load_model(model)
        assert isinstance(model, CompiledModel)
        self.model = model
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BatchSim needs a GPU device (got %s); the HIP path has no CPU fallback" % device)
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be float32 or float64")
        self.dtype = dtype
        self.B = int(batch_size)
        self.tape_capacity = int(tape_capacity)
        L = capi.lib()
        self._I = np.ascontiguousarray(model.I, dtype=np.int32)
        self._F = np.ascontiguousarray(model.F, dtype=np.float64)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        capi.check(L.tsim_batch_create(self._I.ctypes.data_as(capi._ip), self._F.ctypes.data_as(C.POINTER(C.c_double)), self.B,
                                       self.tape_capacity, capi.TSIM_F32 if dtype == torch.float32 else capi.TSIM_F64, idx,
                                       C.byref(h)))
        self._h = h
        self.ndof_r, self.ndof_u = L.tsim_ndof_r(h), L.tsim_ndof_u(h)
        self.ndof_var, self.ndof_tactile = L.tsim_ndof_var(h), L.tsim_ndof_tactile(h)
        self.h = L.tsim_timestep(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                capi.lib().tsim_batch_destroy(h)
            except Exception:
                pass
            self._h = None

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, t, dim, name):
        if t is None:
            return None
        if t.device != self.device or t.dtype != self.dtype:
            t = t.to(device=self.device, dtype=self.dtype)
        t = t.contiguous()
        # env-major [B, dim] (or [B, n, d] with n * d == dim for per-sub-step seeds): a transposed or otherwise mis-shaped
        # tensor must not be reinterpreted silently
        if t.dim() < 2 or t.shape[0] != self.B or t.numel() != self.B * dim:
            raise ValueError("%s: expected shape [%d, %d], got %s" % (name, self.B, dim, tuple(t.shape)))
        return t

    def empty(self, *dims):
        return torch.empty((self.B,) + dims, device=self.device, dtype=self.dtype)

    # ------------------------------------------------------------------ stepping
    def update_model(self, model):
        self.model = model
        self._I = np.ascontiguousarray(model.I, dtype=np.int32)
        self._F = np.ascontiguousarray(model.F, dtype=np.float64)
        capi.check(capi.lib().tsim_update_model(self._h, self._I.ctypes.data_as(capi._ip),
                                                self._F.ctypes.data_as(C.POINTER(C.c_double)), self._stream()))

    # ------------------------------------------------------------------ per-environment parameters
    def base_tables(self):
        """[B, table_size] copy of the model's numeric tables, one row per environment, ready to be edited."""
        n = capi.lib().tsim_table_size(self._h)
        row = torch.tensor(self.model.F[:n], device=self.device, dtype=self.dtype)
        return row.unsqueeze(0).repeat(self.B, 1)

    def set_env_tables(self, tables):
        """Per-environment numeric tables (domain randomisation); None reverts to the shared model."""
        if tables is not None:
            tables = self._chk(tables, capi.lib().tsim_table_size(self._h), "tables")
        capi.check(capi.lib().tsim_set_env_tables(self._h, _ptr(tables), self._stream()))
        self._env_tables = tables      # (the batch reads these rows in every launch: keep them alive)

    def set_param_grad(self, buf):
        """Table gradient (include/tsim.h tsim_set_param_grad): while `buf` ([B, table_size] of the batch's dtype, on its device) is set, every
        backward_steps / backward_episode ADDS dL/d(entry) to it for the columns model.param_columns() names (contact pair and sensor kn kt mu
        damping, dof damping; with set_param_grad_groups also those of model.body_param_columns()) and leaves the other columns untouched.  None switches it off.  The batch keeps a reference to the buffer."""
        if buf is not None:
            n = capi.lib().tsim_table_size(self._h)
            if buf.device != self.device or buf.dtype != self.dtype or tuple(buf.shape) != (self.B, n) or not buf.is_contiguous():
                raise ValueError("set_param_grad: expected a contiguous [%d, %d] %s tensor on %s, got %s %s on %s"
                                 % (self.B, n, self.dtype, self.device, tuple(buf.shape), buf.dtype, buf.device))
        capi.check(capi.lib().tsim_set_param_grad(self._h, _ptr(buf)))
        self._param_grad = buf

    PARAM_GRAD_GROUPS = {"contact": 1, "inertial": 2, "motor": 4, "limit": 8}      # include/tsim.h TSIM_PG_*

    def set_param_grad_groups(self, groups=("contact",)):
        """Which groups of columns set_param_grad's buffer receives (include/tsim.h tsim_set_param_grad_groups): 'contact' (the default:
        model.param_columns()), and the body groups 'inertial', 'motor', 'limit' (model.body_param_columns(): link mass / centre of mass /
        inertia, motor lo hi P D, dof limits).  Takes effect with the next backward launch."""
        mask = 0
        for g in ([groups] if isinstance(groups, str) else groups):
            mask |= self.PARAM_GRAD_GROUPS[g]
        capi.check(capi.lib().tsim_set_param_grad_groups(self._h, mask))

    def param_grad_groups(self):
        mask = capi.lib().tsim_get_param_grad_groups(self._h)
        return tuple(g for g, bit in self.PARAM_GRAD_GROUPS.items() if mask & bit)

    ADJOINT_KERNELS = ("k_backward", "k_backward_z", "k_closed_backward_z")      # include/tsim.h TSIM_ADJ_*

    def last_adjoint_launch(self):
        """What the most recent adjoint launch of this batch ran (include/tsim.h tsim_last_adjoint_launch): {"kernel": "k_backward", its twin
        "k_backward_z" that also saves z (a table-gradient buffer was set), or the closed-loop adjoint's twin "k_closed_backward_z" (None: no adjoint
        launch yet); "param_passes": the passes launched behind it, a tuple out of "k_param_grad", "k_param_grad_body"}."""
        out = (C.c_int32 * 2)()
        capi.check(capi.lib().tsim_last_adjoint_launch(self._h, out))
        return {"kernel": self.ADJOINT_KERNELS[out[0]] if out[0] >= 0 else None,
                "param_passes": tuple(k for i, k in enumerate(("k_param_grad", "k_param_grad_body")) if out[1] >> i & 1)}

    def reset(self, q0, qd0=None, backward_flag=False):
        q0 = self._chk(q0, self.ndof_r, "q0")
        qd0 = self._chk(qd0, self.ndof_r, "qd0")
        capi.check(capi.lib().tsim_reset(self._h, _ptr(q0), _ptr(qd0), int(bool(backward_flag)), self._stream()))

    def reset_masked(self, q0, mask, qd0=None):
        """New state for the environments with mask != 0 only (forward-only batches: roll-out collection)."""
        q0 = self._chk(q0, self.ndof_r, "q0")
        qd0 = self._chk(qd0, self.ndof_r, "qd0")
        m = torch.as_tensor(mask).to(device=self.device).reshape(-1)
        if m.numel() != self.B:
            raise ValueError("mask: expected %d entries" % self.B)
        m = (m != 0).to(torch.int32).contiguous()
        capi.check(capi.lib().tsim_reset_masked(self._h, _ptr(q0), _ptr(qd0), _ptr(m), self._stream()))

    def step(self, u, num_steps=1, want_qd=False, want_var=True, want_tactile=True, out=None):
        """One env-step for all B environments. Returns dict(q, qd, var, tactile, status)."""
        u = self._chk(u, self.ndof_u, "u")
        o = out if out is not None else {}
        if "q" not in o:
            o["q"] = self.empty(self.ndof_r)
        if want_qd and "qd" not in o:
            o["qd"] = self.empty(self.ndof_r)
        if want_var and self.ndof_var and "var" not in o:
            o["var"] = self.empty(self.ndof_var)
        if want_tactile and self.ndof_tactile and "tactile" not in o:
            o["tactile"] = self.empty(self.ndof_tactile)
        if "status" not in o:
            o["status"] = torch.empty(self.B, device=self.device, dtype=torch.int32)
        capi.check(capi.lib().tsim_step(self._h, _ptr(u), int(num_steps), _ptr(o["q"]), _ptr(o.get("qd")), _ptr(o.get("var")),
                                        _ptr(o.get("tactile")), _ptr(o["status"]), self._stream()))
        return o

    def _tactile_slots(self, T, tactile_mask):
        """tactile_masks (bool[T]) of EpisodicSimFunction -> (device int32[T] slot map, number of masked frames)."""
        if tactile_mask is None:
            return None, T
        m = torch.as_tensor(tactile_mask).to(device=self.device).reshape(-1).bool()
        if m.numel() != T:
            raise ValueError("tactile_mask: expected %d entries, got %d" % (T, m.numel()))
        slots = torch.where(m, torch.cumsum(m.int(), 0) - 1, torch.full_like(m, -1, dtype=torch.int64)).to(torch.int32).contiguous()
        return slots, int(m.sum().item())

    def rollout(self, u, num_steps=1, want_qd=False, want_var=True, want_tactile=True, tactile_mask=None):
        """Open-loop episode in one launch (include/tsim.h tsim_rollout): u [T, B, ndof_u] -> dict of [T, B, dim] outputs
        (+ status [B]); the same results as T calls of step().  tactile_mask (bool[T]): tactile only for the masked
        frames, output [n_masked, B, ndof_tactile]."""
        if u.dim() != 3 or u.shape[1] != self.B or u.shape[2] != self.ndof_u:
            raise ValueError("rollout: u must be [T, %d, %d], got %s" % (self.B, self.ndof_u, tuple(u.shape)))
        T = int(u.shape[0])
        u = u.to(device=self.device, dtype=self.dtype).contiguous()
        new = lambda d: torch.empty((T, self.B, d), device=self.device, dtype=self.dtype)
        o = {"q": new(self.ndof_r), "status": torch.empty(self.B, device=self.device, dtype=torch.int32)}
        if want_qd:
            o["qd"] = new(self.ndof_r)
        if want_var and self.ndof_var:
            o["var"] = new(self.ndof_var)
        slots, nm = self._tactile_slots(T, tactile_mask)
        if want_tactile and self.ndof_tactile:
            o["tactile"] = torch.empty((nm, self.B, self.ndof_tactile), device=self.device, dtype=self.dtype)
        capi.check(capi.lib().tsim_rollout(self._h, _ptr(u), T, int(num_steps), _ptr(slots), _ptr(o["q"]), _ptr(o.get("qd")),
                                           _ptr(o.get("var")), _ptr(o.get("tactile")), _ptr(o["status"]), self._stream()))
        return o

    def backward_episode(self, num_frames, num_steps, df_dq=None, df_dvar=None, df_dtactile=None, tactile_mask=None):
        """Adjoint of the newest num_frames env-steps (num_steps sub-steps each) in one launch. Seeds [T, B, dim] or None
        (df_dtactile [n_masked, B, dim] with tactile_mask); returns df_du [T, B, ndof_u] (gradient w.r.t. the action of
        each frame)."""
        T = int(num_frames)
        slots, nm = self._tactile_slots(T, tactile_mask)

        def chk(t, dim, name, n=T):
            if t is None or dim == 0:
                return None
            t = t.to(device=self.device, dtype=self.dtype).contiguous()
            if tuple(t.shape) != (n, self.B, dim):
                raise ValueError("%s: expected [%d, %d, %d], got %s" % (name, n, self.B, dim, tuple(t.shape)))
            return t
        a, b = chk(df_dq, self.ndof_r, "df_dq"), chk(df_dvar, self.ndof_var, "df_dvar")
        c = chk(df_dtactile, self.ndof_tactile, "df_dtactile", nm) if nm > 0 else None
        du = torch.empty((T, self.B, self.ndof_u), device=self.device, dtype=self.dtype)
        capi.check(capi.lib().tsim_backward_episode(self._h, T, int(num_steps), _ptr(slots), _ptr(a), _ptr(b), _ptr(c), _ptr(du),
                                                    self._stream()))
        return du

    TANGENT_MAX_DIR = 8      # include/tsim.h TSIM_TANGENT_MAX_DIR

    def tangent_episode(self, num_frames, num_steps, du=None, dq0=None, dqd0=None, dtables=None, tactile_mask=None, want_qd=False, want_var=True,
                        want_tactile=True):
        """Forward-mode tangent of the newest num_frames env-steps (num_steps sub-steps each) in one launch (include/tsim.h tsim_tangent_episode):
        J v where backward_episode + get_adjoint + set_param_grad give J^T w.  Directions, leading dimension ndir (1 .. 8, taken from the inputs
        given, which must agree; all None: one zero direction): du [ndir, T, B, ndof_u], dq0 / dqd0 [ndir, B, ndof_r] (the tangent of the state
        at the window's start), dtables [ndir, B, table_size] (the columns of model.param_columns() are read, and those of
        model.body_param_columns() whose group — 'inertial', 'motor', 'limit' — is on in set_param_grad_groups; no other entry, and with the default
        groups a body column changes no output bit.  The first call with a body group on, or one larger than any before, allocates the batch's
        workspace for the body term and synchronises; capture a launch only after such a warm-up call).  Returns a dict dq [ndir, T, B,
        ndof_r], dqd (want_qd), dvar [ndir, T, B, ndof_var], dtactile [ndir, n_masked, B, ndof_tactile].  The tape, the state and the carried adjoint
        are left as they are."""
        T = int(num_frames)
        slots, nm = self._tactile_slots(T, tactile_mask)
        ntab = capi.lib().tsim_table_size(self._h)
        ndir = None
        ins = []
        for t, tail, name in ((du, (T, self.B, self.ndof_u), "du"), (dq0, (self.B, self.ndof_r), "dq0"), (dqd0, (self.B, self.ndof_r), "dqd0"),
                              (dtables, (self.B, ntab), "dtables")):
            if t is None:
                ins.append(None)
                continue
            t = t.to(device=self.device, dtype=self.dtype).contiguous()
            if t.dim() != len(tail) + 1 or tuple(t.shape[1:]) != tail:
                raise ValueError("%s: expected [ndir, %s], got %s" % (name, ", ".join(str(x) for x in tail), tuple(t.shape)))
            if ndir is not None and t.shape[0] != ndir:
                raise ValueError("%s: %d directions, the other inputs have %d" % (name, t.shape[0], ndir))
            ndir = int(t.shape[0])
            ins.append(t if t.numel() else None)
        ndir = 1 if ndir is None else ndir
        if not 1 <= ndir <= self.TANGENT_MAX_DIR:
            raise ValueError("tangent_episode: 1 .. %d directions per launch, got %d" % (self.TANGENT_MAX_DIR, ndir))
        new = lambda n, d: torch.empty((ndir, n, self.B, d), device=self.device, dtype=self.dtype)
        o = {"dq": new(T, self.ndof_r)}
        if want_qd:
            o["dqd"] = new(T, self.ndof_r)
        if want_var and self.ndof_var:
            o["dvar"] = new(T, self.ndof_var)
        if want_tactile and self.ndof_tactile:
            o["dtactile"] = new(nm, self.ndof_tactile)
        capi.check(capi.lib().tsim_tangent_episode(self._h, T, int(num_steps), ndir, _ptr(slots), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]),
                                                   _ptr(o["dq"]), _ptr(o.get("dqd")), _ptr(o.get("dvar")), _ptr(o.get("dtactile")), self._stream()))
        return o

    def frame_jacobians(self, num_frames, num_steps, want_A=True, want_B=True, want_var=False):
        """Per-frame transition Jacobians of the newest num_frames env-steps (num_steps sub-steps each) in one launch (include/tsim.h
        tsim_frame_jacobians), with x = (q, qd): a dict of A [T, B, 2 ndof_r, 2 ndof_r] = dx_{f+1} / dx_f (want_A), B [T, B, 2 ndof_r, ndof_u] =
        dx_{f+1} / du_f with u held for the frame (want_B; a clipped force control: exactly zero columns) and Jvar [T, B, ndof_var, ndof_r] =
        dvariables / dq at the frame's end state (want_var).  BDF1 models only.  The tape, the state and the carried adjoint are left as they
        are; a frame's matrices do not depend on num_frames or on which of A, B are asked for."""
        T = int(num_frames)
        n2 = 2 * self.ndof_r
        new = lambda r, c: torch.empty((T, self.B, r, c), device=self.device, dtype=self.dtype)
        o = {}
        if want_A:
            o["A"] = new(n2, n2)
        if want_B:
            o["B"] = new(n2, self.ndof_u)
        if want_var and self.ndof_var:
            o["Jvar"] = new(self.ndof_var, self.ndof_r)
        capi.check(capi.lib().tsim_frame_jacobians(self._h, T, int(num_steps), _ptr(o.get("A")), _ptr(o.get("B")), _ptr(o.get("Jvar")), self._stream()))
        return o

    def tactile_jacobians(self, num_frames, num_steps, tactile_mask=None):
        """Per-frame tactile Jacobians of the newest num_frames env-steps (num_steps sub-steps each) in one launch (include/tsim.h
        tsim_tactile_jacobians): Ct [n_masked, B, 2 ndof_r, ndof_tactile], the TRANSPOSE of C_f = dtactile / d(q, qd) at the frame's end state —
        row d is column d of C_f as one tactile frame (rows < ndof_r: d/dq, the rest: d/dqd); functions.episode_observation gives the view
        [.., ndof_tactile, 2 ndof_r].  tactile_mask (bool[T]) as in rollout: only the masked frames are computed and stored, and a mask without
        a masked frame is refused.  An unloaded taxel gives exact zeros.  BDF2 and rotation-vector models are accepted.  The tape, the state and
        the carried adjoint are left as they are; a frame's bits do not depend on num_frames, the mask or the batch size.
        Size: 2 ndof_r * ndof_tactile reals per environment and masked frame — TactilePush fp32 21 840 bytes (20 frames x 4096 environments:
        1.79 GB), D'Claw 217 440 bytes (20 x 2048: 8.9 GB): mask the frames that are needed."""
        T = int(num_frames)
        slots, nm = self._tactile_slots(T, tactile_mask)
        if nm < 1:
            raise ValueError("tactile_jacobians: the mask has no masked frame")
        Ct = torch.empty((nm, self.B, 2 * self.ndof_r, self.ndof_tactile), device=self.device, dtype=self.dtype)
        capi.check(capi.lib().tsim_tactile_jacobians(self._h, T, int(num_steps), _ptr(slots), _ptr(Ct), self._stream()))
        return Ct

    PARAM_JACOBIAN_MAX_COLS = 32      # TSIM_PARAM_JACOBIAN_MAX_COLS of include/tsim.h

    def param_jacobians(self, num_frames, num_steps, cols, want_E=True, want_tactile=False, tactile_mask=None):
        """Per-frame parameter Jacobians of the newest num_frames env-steps (num_steps sub-steps each) in one launch (include/tsim.h
        tsim_param_jacobians), with x = (q, qd) and p the environment's contact-group parameters: a dict of E [T, B, 2 ndof_r, len(cols)] =
        dx_{f+1} / dp at fixed (x_f, u_f) (want_E; cols: 1 .. 32 table columns out of model.param_columns(), each once; BDF1 models only) and Ft
        [n_masked, B, 4, ndof_tactile] = dtactile / dp at fixed x_{f+1} (want_tactile), stored compactly: row k is the derivative of every taxel
        w.r.t. field k (kn, kt, mu, damping) of its OWN sensor; functions.episode_parameters scatters it to the dense F.  tactile_mask (bool[T]) as
        in tactile_jacobians, for Ft only; a mask without a masked frame is refused.  Sensor columns, sensing-only pairs and pairs out of contact
        give exactly zero columns of E; unloaded taxels exact zeros in Ft.  The tape, the state and the carried adjoint are left as they are; a
        column's bits depend neither on the other columns nor on num_frames, want_tactile or the batch size."""
        T = int(num_frames)
        o = {}
        ncols, carr = 0, None
        if want_E:
            cols = [int(x) for x in cols]
            ncols = len(cols)
            carr = (C.c_int32 * max(ncols, 1))(*cols)
            o["E"] = torch.empty((T, self.B, 2 * self.ndof_r, ncols), device=self.device, dtype=self.dtype)
        slots = None
        if want_tactile:
            slots, nm = self._tactile_slots(T, tactile_mask)
            if nm < 1:
                raise ValueError("param_jacobians: the mask has no masked frame")
            o["Ft"] = torch.empty((nm, self.B, 4, self.ndof_tactile), device=self.device, dtype=self.dtype)
        capi.check(capi.lib().tsim_param_jacobians(self._h, T, int(num_steps), ncols, carr, _ptr(slots), _ptr(o.get("E")), _ptr(o.get("Ft")), self._stream()))
        return o

    def tactile_normal_equations(self, num_frames, num_steps, weight=None, residual=None, with_params=False, tactile_mask=None):
        """The information form of the tactile block of the newest num_frames env-steps (num_steps sub-steps each) in one launch (include/tsim.h
        tsim_tactile_normal_equations): a dict of N [n_masked, B, Z, Z] = H^T W H and, with `residual`, n [n_masked, B, Z] = H^T W r, for
        H = [C_f | F_f] — C_f of tactile_jacobians, F_f the dense form of param_jacobians' Ft (with_params: column 2 ndof_r + 4 s + k is field k
        = kn, kt, mu, damping of sensor s), Z = 2 ndof_r + (4 nsensor if with_params) — without C_f or F_f being stored.  weight [ndof_tactile]:
        the diagonal of W, shared by all environments and frames (None: ones; negative or non-finite values are the caller's business);
        residual [n_masked, B, ndof_tactile].  Both must be on the batch's device in its dtype and contiguous.  tactile_mask (bool[T]) as in
        tactile_jacobians; a mask without a masked frame is refused.  N is exactly symmetric; a frame without a loaded taxel gives zeros, a sensor
        without one zero parameter rows and columns.  The tape, the state and the carried adjoint are left as they are; a frame's bits do not
        depend on num_frames, the mask or the batch size, the state block's neither on with_params nor on residual.
        Size: Z^2 + Z reals per environment and masked frame — TactilePush with parameters, fp32: 1 368 bytes (Ct and Ft: 27 300)."""
        T = int(num_frames)
        ntac = self.ndof_tactile
        for name, t in (("weight", weight), ("residual", residual)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != self.dtype or not t.is_contiguous():
                raise ValueError("tactile_normal_equations: %s must be a contiguous %s tensor on %s" % (name, self.dtype, self.device))
        slots, nm = self._tactile_slots(T, tactile_mask)
        if nm < 1:
            raise ValueError("tactile_normal_equations: the mask has no masked frame")
        if weight is not None and tuple(weight.shape) != (ntac,):
            raise ValueError("tactile_normal_equations: weight: expected shape [%d], got %s" % (ntac, tuple(weight.shape)))
        if residual is not None and tuple(residual.shape) != (nm, self.B, ntac):
            raise ValueError("tactile_normal_equations: residual: expected shape [%d, %d, %d], got %s" % (nm, self.B, ntac, tuple(residual.shape)))
        Z = 2 * self.ndof_r + (4 * int(self.model.I[_blob.TSIM_IH_NSENSOR]) if with_params else 0)
        o = {"N": torch.empty((nm, self.B, Z, Z), device=self.device, dtype=self.dtype)}
        if residual is not None:
            o["n"] = torch.empty((nm, self.B, Z), device=self.device, dtype=self.dtype)
        capi.check(capi.lib().tsim_tactile_normal_equations(self._h, T, int(num_steps), _ptr(slots), int(bool(with_params)), _ptr(weight), _ptr(residual),
                                                            _ptr(o["N"]), _ptr(o.get("n")), self._stream()))
        return o

    def get_state(self):
        q, qd =self.empty(self.ndof_r), self.empty(self.ndof_r)
        capi.check(capi.lib().tsim_get_state(self._h, _ptr(q), _ptr(qd), self._stream()))
        return q, qd

    def readout(self, want_var=True, want_tactile=True):
        var = self.empty(self.ndof_var) if (want_var and self.ndof_var) else None
        tac = self.empty(self.ndof_tactile) if (want_tactile and self.ndof_tactile) else None
        if var is not None or tac is not None:
            capi.check(capi.lib().tsim_readout(self._h, _ptr(var), _ptr(tac), self._stream()))
        return var, tac

    # ------------------------------------------------------------------ adjoint
    def backward_steps(self, n, df_dq=None, df_dvar=None, df_dtactile=None, all_steps=False):
        """Adjoint of the newest n recorded sub-steps. Seeds are [B, dim] (last sub-step only) or, with
        all_steps=True, [B, n, dim]. Returns df_du [B, n, ndof_u]."""
        mul = n if all_steps else 1
        a = self._chk(df_dq, mul * self.ndof_r, "df_dq")
        b = self._chk(df_dvar, mul * self.ndof_var, "df_dvar") if self.ndof_var else None
        c = self._chk(df_dtactile, mul * self.ndof_tactile, "df_dtactile") if self.ndof_tactile else None
        du = self.empty(n, self.ndof_u)
        capi.check(capi.lib().tsim_backward_steps(self._h, int(n), int(bool(all_steps)), _ptr(a), _ptr(b), _ptr(c), _ptr(du),
                                                  self._stream()))
        return du

    def get_adjoint(self):
        a, b = self.empty(self.ndof_r), self.empty(self.ndof_r)
        capi.check(capi.lib().tsim_get_adjoint(self._h, _ptr(a), _ptr(b), self._stream()))
        return a, b

    def tape_len(self):
        return capi.lib().tsim_tape_len(self._h)

    def cache_save(self):
        capi.check(capi.lib().tsim_cache_save(self._h, self._stream()))

    def cache_pop(self):
        capi.check(capi.lib().tsim_cache_pop(self._h, self._stream()))

    def cache_clear(self):
        capi.check(capi.lib().tsim_cache_clear(self._h))

    def cache_reserve(self, depth):
        """Pre-allocate tape buffers for `depth` saved episodes, so that cache_save / cache_pop never allocate."""
        capi.check(capi.lib().tsim_cache_reserve(self._h, int(depth)))

    def cache_depth(self):
        return capi.lib().tsim_cache_depth(self._h)

    # ------------------------------------------------------------------ diagnostics
    def debug_eval(self, q1, q0, qd0, u, cycles=False):
        q1, q0, qd0 = (self._chk(x, self.ndof_r, "q") for x in (q1, q0, qd0))
        u = self._chk(u, self.ndof_u, "u")
        g, H = self.empty(self.ndof_r), self.empty(self.ndof_r, self.ndof_r)
        cyc = torch.zeros(self.B, 32, device=self.device, dtype=torch.int64) if cycles else None
        capi.check(capi.lib().tsim_debug_eval(self._h, _ptr(q1), _ptr(q0), _ptr(qd0), _ptr(u), _ptr(g), _ptr(H), _ptr(cyc),
                                              self._stream()))
        return (g, H, cyc) if cycles else (g, H)

    def branch_signature(self, t_first=0, n=None):
        """[n, B, 2] int64 (count, hash) of the contact / friction branches of the taped sub-steps t_first+1 .. t_first+n
        (include/tsim.h tsim_debug_signature); needs reset(backward_flag=True)."""
        n = self.tape_len() - t_first if n is None else int(n)
        out = torch.empty((n, self.B, 2), device=self.device, dtype=torch.int32)
        capi.check(capi.lib().tsim_debug_signature(self._h, int(t_first), n, _ptr(out), self._stream()))
        return out.to(torch.int64) & 0xFFFFFFFF

    def last_evals(self):
        out = np.zeros(self.B, dtype=np.int32)
        capi.check(capi.lib().tsim_last_evals(self._h, out.ctypes.data_as(capi._ip)))
        return out

    def last_helper_trials(self):
        """Line-search trials of the most recent forward launch that a helper slot evaluated, per environment (include/tsim.h TSIM_OPT_TRIAL_HELPERS)."""
        out = np.zeros(self.B, dtype=np.int32)
        capi.check(capi.lib().tsim_last_helper_trials(self._h, out.ctypes.data_as(capi._ip)))
        return out

    def last_gnorm(self):
        """Largest ||g|| any sub-step of the most recent forward launch ended with, per environment (float32 [B])."""
        out = np.zeros(self.B, dtype=np.float32)
        capi.check(capi.lib().tsim_last_gnorm(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def set_solver_options(self, cross_kinks=None, eval_budget=0):
        """include/tsim.h tsim_set_solver_options: the two options around the XML-stated Newton loop.  cross_kinks None = the library's
        default (on for fp32 batches, off for fp64 ones, which then run the literal loop)."""
        if cross_kinks is None:
            cross_kinks = self.dtype == torch.float32
        capi.check(capi.lib().tsim_set_solver_options(self._h, int(bool(cross_kinks)), int(eval_budget)))

    def set_lanes_per_env(self, lanes):
        """16 / 32 / 64 lanes per environment, 0 = automatic (include/tsim.h tsim_set_lanes_per_env)."""
        capi.check(capi.lib().tsim_set_lanes_per_env(self._h, int(lanes)))

    def static_model(self):
        """Id of the statically specialised kernel instantiation the next launch uses (include/tsim.h tsim_static_model; 0: generic)."""
        return capi.lib().tsim_static_model(self._h)

    def set_static(self, allow):
        capi.check(capi.lib().tsim_set_static(self._h, int(bool(allow))))

    def kernel_variant(self):
        """Name of the kernel instantiation the next launch uses: "generic", "static:<model>", "param:<model>" (include/tsim.h)."""
        return capi.lib().tsim_kernel_variant(self._h).decode()

    OPT_PAIR_CULL, OPT_VALUE_TRIALS, OPT_TRIAL_HELPERS, OPT_VALUE_FIRST, OPT_CROSS_KINKS, OPT_EVAL_BUDGET, OPT_ALL_DEFAULT, OPT_FRAME_RECORDS = 1, 2, 3, 4, 5, 6, 7, 8
    OPT_FORWARD_SPLIT = 9      # read-only: the newest forward launch went out split by LPT rank (include/tsim.h)
    OPT_PREDICTOR_HELPERS = 10      # finished slots evaluate a live slot's next predictor ahead (include/tsim.h; TSIM_NO_PREDICTOR_HELPERS=1 at creation: off)
    OPT_ADJOINT_PREPASS = 11      # set: the episode adjoint's seed pre-pass on / off; get: the last adjoint launch took it (include/tsim.h; TSIM_NO_ADJOINT_PREPASS=1 at creation: off)

    def set_option(self, option, value):
        """include/tsim.h tsim_set_option (TSIM_OPT_*)."""
        capi.check(capi.lib().tsim_set_option(self._h, int(option), int(value)))

    def get_option(self, option):
        return capi.lib().tsim_get_option(self._h, int(option))

    KERNEL_KINDS = ("k_forward", "k_taxels", "k_backward")

    def kernel_timing(self, enable=True):
        """HIP events around every simulation-kernel launch of this batch, on the launching stream (include/tsim.h tsim_kernel_timing)."""
        capi.check(capi.lib().tsim_kernel_timing(self._h, int(bool(enable))))

    def kernel_times(self):
        """{kernel: (summed ms, launches)} since the previous call; waits for the recorded events (include/tsim.h tsim_kernel_times)."""
        ms, n = (C.c_double * 3)(), (C.c_int32 * 3)()
        capi.check(capi.lib().tsim_kernel_times(self._h, ms, n))
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(self.KERNEL_KINDS)}

    def launch_info(self):
        out = (C.c_int32 * 4)()
        capi.lib().tsim_launch_info(self._h, out)
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}

    def tangent_launch_info(self, ndir=8, with_dtables=True):
        """launch_info() of a tangent_episode call of ndir directions (include/tsim.h tsim_tangent_launch_info): its lanes per environment may be
        wider than the batch's, where a block would not hold the tangent state of eight directions"""
        out = (C.c_int32 * 4)()
        capi.check(capi.lib().tsim_tangent_launch_info(self._h, int(ndir), int(bool(with_dtables)), out))
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}

    def frame_jacobians_launch_info(self):
        """launch_info() of a frame_jacobians call (include/tsim.h tsim_frame_jacobians_launch_info): blocks PER FRAME; its lanes per environment
        may be wider than the batch's, where a block would not hold the 2 ndof_r + ndof_u columns of every slot"""
        out = (C.c_int32 * 4)()
        capi.check(capi.lib().tsim_frame_jacobians_launch_info(self._h, out))
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}

    def tactile_jacobians_launch_info(self):
        """launch_info() of a tactile_jacobians call (include/tsim.h tsim_tactile_jacobians_launch_info): blocks PER FRAME; its lanes per
        environment may be wider than the batch's, where a block would not hold a pair's 18 ndof_r record reals of every slot"""
        out = (C.c_int32 * 4)()
        capi.check(capi.lib().tsim_tactile_jacobians_launch_info(self._h, out))
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}

    def param_jacobians_launch_info(self):
        """launch_info() of a param_jacobians call (include/tsim.h tsim_param_jacobians_launch_info): blocks PER FRAME; its lanes per
        environment may be wider than the batch's, where a block would not hold the 32 columns of every slot; they depend neither on the
        columns selected nor on the outputs asked for"""
        out = (C.c_int32 * 4)()
        capi.check(capi.lib().tsim_param_jacobians_launch_info(self._h, out))
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}

    def tactile_normal_equations_launch_info(self, with_params=False):
        """launch_info() of a tactile_normal_equations call (include/tsim.h tsim_tactile_normal_equations_launch_info): blocks PER FRAME; its
        lanes per environment may be wider than the batch's, where a block would not hold every slot's records, sums and row tile; they depend
        on with_params and on nothing else of a call"""
        out = (C.c_int32 * 4)()
        capi.check(capi.lib().tsim_tactile_normal_equations_launch_info(self._h, int(bool(with_params)), out))
        return {"lds_bytes": out[0], "threads": out[1], "blocks": out[2], "lanes_per_env": out[3]}
