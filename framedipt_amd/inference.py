"""Reverse-diffusion driver with the signature of ``experiments/utils.py:inference_fn`` (:511-626).

Python drives the loop; a step is two C-ABI calls (score-network forward, fused SE(3) reverse step) on one HIP stream, addressed
through a device-side step cursor so that a step is captured once as a HIP graph and replayed (``ReverseLoop``).  Nothing
crosses to the host inside the loop: the state (x_t, self-conditioning CA, trajectories) stays in HBM and the noise tape /
per-step scalars are uploaded up front (the reference does >= 5 device->host syncs per step, SURVEY.md section 0 finding 3).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, gpu_guard
from . import noise as noise_mod
from .model.score_network import preprocess_aatype


def draw_noise_tape(diffuser, n_steps: int, B: int, N: int):
    """Noise of the reverse steps from the global legacy ``np.random`` stream in the reference's order
    (per step: SO(3) draw ``so3_diffuser.py:590`` then R^3 draw ``r3_diffuser.py:371``, each [B,N,3])."""
    z_rot = np.zeros((n_steps, B, N, 3))
    z_trans = np.zeros((n_steps, B, N, 3))
    for s in range(n_steps):
        if diffuser._diffuse_rot:
            z_rot[s] = np.random.normal(size=(B, N, 3))
        if diffuser._diffuse_trans:
            z_trans[s] = np.random.normal(size=(B, N, 3))
    return z_rot, z_trans


def kept_steps(num_t: int, keep="all") -> np.ndarray:
    """The reverse steps k (ascending) whose frames a trajectory of ``num_t`` steps keeps: ``"all"`` every step, ``"last"`` the final one, an
    integer stride ``s >= 1`` the steps with ``(num_t - 1 - k) % s == 0`` — the final step ``num_t - 1`` is always among them, so that row 0
    of every returned (flipped) array is the sample.  The one rule of ``keep=``: buffers, row maps and returned arrays all come from here."""
    num_t = int(num_t)
    if num_t < 1:
        raise ValueError(f"num_t = {num_t}: a trajectory has at least one step")
    k = np.arange(num_t, dtype=np.int64)
    if isinstance(keep, str):
        if keep == "all":
            return k
        if keep == "last":
            return k[-1:]
        raise ValueError(f"keep={keep!r}: expected 'all', 'last' or an integer stride >= 1")
    if isinstance(keep, (bool, np.bool_)) or not isinstance(keep, (int, np.integer)):
        raise ValueError(f"keep={keep!r}: expected 'all', 'last' or an integer stride >= 1")
    if keep < 1:
        raise ValueError(f"keep={keep}: the stride must be >= 1")
    return k[(num_t - 1 - k) % int(keep) == 0]


def _aatype_views(model, data_init, fixed, inpainting, input_aatype, dev):
    """(aatype of the trajectory frames, aatype the network sees, are they the same): see ``ReverseLoop.__init__``."""
    to_dev = lambda x: None if x is None else x.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    aatype = to_dev(preprocess_aatype(data_init.get("aatype"), fixed, inpainting, input_aatype))
    net_aatype = to_dev(preprocess_aatype(data_init.get("aatype"), fixed, model.inpainting, model._model_conf.input_aatype))
    same = (aatype is None and net_aatype is None) or (
        aatype is not None and net_aatype is not None and bool(torch.equal(aatype, net_aatype)))
    return aatype, net_aatype, same


def _backbone(net, n, t7, rot, trans, psi, aatype, atom37):
    lib = _lib.load()
    _lib.check(lib.fdipt_backbone_atoms(n, _lib.ptr(t7), _lib.ptr(rot), _lib.ptr(trans), _lib.ptr(psi), _lib.ptr(aatype),
                                        _lib.ptr(net.bb_tables), _lib.ptr(atom37), None, _lib.stream_ptr()),
               "backbone_atoms")


def get_atom_positions_from_rigids(model, rigids, psi_torsions, aatype=None) -> np.ndarray:
    """``experiments/utils.py:415-437``: backbone atom37 positions [B,N,37,3] (NumPy) of frames given as tensor_7 [B,N,7] (or a
    ``Rigid``), psi torsions [B,N,2] and residue types [B,N] (None: alanine), through the backbone kernel."""
    t7 = rigids.to_tensor_7() if hasattr(rigids, "to_tensor_7") else rigids
    dev = model.device
    with torch.cuda.device(dev):
        t7 = t7.to(device=dev, dtype=torch.float32).contiguous()
        psi = psi_torsions.to(device=dev, dtype=torch.float32).contiguous()
        aa = None if aatype is None else aatype.to(device=dev, dtype=torch.int32).contiguous()
        atom37 = torch.empty(t7.shape[:-1] + (37, 3), dtype=torch.float32, device=dev)
        _backbone(model, int(np.prod(t7.shape[:-1])), t7, None, None, psi, aa, atom37)
        return atom37.cpu().numpy()


class ReverseLoop:
    """Device-resident state of one batch of trajectories; ``run()``, or ``prime()`` then ``step(k)`` for k = 0..num_t-1.

    **Step graph (the default, ``graph=True``).**  Every reverse step but the last is the same ~70 kernel launches on different
    rows of the trajectory arrays.  The library addresses those rows through a device-side step cursor
    (``FdiptForwardArgs.step_cursor``, ``fdipt_se3_reverse_step_indexed``: the fused reverse step advances it), so the launch
    arguments of a step do not depend on the step: the first noisy step is enqueued eagerly through the cursor (it also runs every
    kernel once), the second one is captured as a HIP graph — and ``GRAPH_CHUNK`` consecutive steps as a second graph — and all
    later steps are replays: one ``hipGraphLaunch`` per chunk instead of ~67 ``hipLaunchKernel`` + 3 ctypes calls per step
    (0.09 ms against 0.24 ms of host work per 2.1 - 2.2 ms GPU step at N = 300, B = 8 on a quiet host; under any per-call overhead —
    a tracer costs 45 us per launch — only the replayed loop stays GPU-bound: profiles/r05_driver_cmd_repro.md).  Same kernels, same
    bits as the eager loop (``graph=False``; tests/test_gpu_round5.py, tools/soak_step_graph.py).  The graphs hold pointers into this
    loop's buffers and its ``BatchState``: they live and die with the loop — and serve every batch the loop is ``reset()`` to.

    **Kept frames (``keep=``, opt-in).**  ``"all"`` (default) materialises every step's frames, as the reference's trajectories do.
    ``"last"`` / a stride (``kept_steps``) sizes ``prot_traj`` / ``bb0_traj`` / ``trans_traj`` and the kept rigid rows to the kept steps
    only; the state then lives in a two-row ring (x_t of step k = row ``k & 1``) and a device row map (``frame_rows``: step -> kept row
    or -1) tells the cursor-addressed launches where a step's frames go — or that the step builds none.  The launch sequence stays
    independent of the step, so one captured graph still serves every step; the frames that are kept are bit-identical to the
    ``keep="all"`` run's (tests/test_gpu_kept_frames.py)."""

    GRAPH_CHUNK = 8  # steps per replay of the chunk graph (``run()``); single steps replay the one-step graph

    def __init__(self, model, diffuser, data_init, num_t, min_t, center=True, aux_traj=False, self_condition=True,
                 noise_scale=1.0, embed_self_conditioning=True, inpainting=False, input_aatype=False, noise_tape=None, state=None,
                 graph=True, verify=0, noise="host", noise_keys=None, keep="all"):
        self.model, self.diffuser = model, diffuser
        self.keep = keep
        steps = kept_steps(num_t, keep)     # (raises on a bad value before anything is allocated)
        self.kept = keep != "all"           # kept-frame addressing: row map + two-row state (keep=1 keeps every step through it)
        # noise="device": no tape is drawn or uploaded, the reverse-step kernel draws from the samples' keys (noise.py)
        keys = noise_mod.resolve(noise, noise_keys, noise_tape, int(data_init["rigids_t"].shape[0]))
        dev = self.dev = model.device
        gpu_guard.check(dev, what="inference_fn")  # a foreign compute process on this GPU: warn / refuse (FDIPT_SHARED_GPU)
        self.verify, self.verified = int(verify or 0), 0
        rig0 = data_init["rigids_t"]
        _lib.require_cuda(rig0, "inference_fn")
        if rig0.dim() == 2:
            raise ValueError("rigids_t needs a leading batch dimension")
        B, N = self.B, self.N = rig0.shape[0], rig0.shape[1]
        f32 = lambda x: x.to(device=dev, dtype=torch.float32).contiguous().clone()  # noqa: E731
        self.res_mask, self.fixed = f32(data_init["res_mask"]), f32(data_init["fixed_mask"])
        self.fixed_mask = (self.fixed * self.res_mask).contiguous()
        self.diffuse_mask = ((1 - self.fixed) * self.res_mask).contiguous()
        # two aatype views, as in the reference: the network pre-processes with ITS OWN flags (score_network.py:226-232:
        # self.inpainting / model_conf.input_aatype), the atom37 frames of the trajectory with inference_fn's arguments
        # (experiments/utils.py:376-388)
        self._inpainting, self._input_aatype = inpainting, input_aatype
        self.aatype, self.net_aatype, same = _aatype_views(model, data_init, self.fixed, inpainting, input_aatype, dev)
        # rigid_0_traj (bb_0_pred, experiments/utils.py:397-402) is built with inference_fn's aatype.  Where that equals the
        # network's own view the forward writes the row itself; where it does not (the reference's default inpainting
        # configuration: inference.input_aatype=True with model.input_aatype=False, so the network sees 20 = unknown on the
        # diffused residues and would build ALA there) the row comes from a backbone launch on the forward's frames / psi
        # (net_aatype None = the backbone builder's default residue 0, as is aatype None)
        self.bb0_from_forward = same
        self.gt_tors = data_init["torsion_angles_sin_cos"]
        self.gt_psi = f32(self.gt_tors[..., 2, :])
        self.st = state if state is not None else model.batch_state(data_init["seq_idx"])
        self.num_t, self.min_t, self.dt = num_t, min_t, 1 / num_t
        self.center, self.aux_traj, self.noise_scale = center, aux_traj, noise_scale
        self.self_condition, self.embed_sc = self_condition, embed_self_conditioning
        self.reverse_steps = np.linspace(min_t, 1.0, num_t)[::-1]
        # steps that take the reverse SDE step (t > min_t): a prefix of the schedule (it decreases to min_t)
        n_noisy = self.n_noisy = int(np.sum(self.reverse_steps > min_t))
        t32, temb, sig = model.step_scalars(self.reverse_steps)
        with torch.cuda.device(dev):
            self.t_all = torch.as_tensor(np.repeat(t32[:, None], B, 1), device=dev)
            self.temb_all = torch.as_tensor(np.repeat(temb[:, None, :], B, 1), device=dev)
            self.sig_all = torch.as_tensor(np.repeat(sig[:, None], B, 1), device=dev)
            self.t_tab = torch.as_tensor(np.ascontiguousarray(self.reverse_steps, dtype=np.float64), device=dev)
            so3 = diffuser._so3_diffuser
            self.tab_all = self.omega_edges = None
            if so3.use_cached_score:  # one row of the score-norm table per step (all samples of a batch share t)
                rows = so3.score_table_rows(t32)
                self.tab_all = torch.as_tensor(np.repeat(rows[:, None, :], B, 1), device=dev)
                self.omega_edges = torch.as_tensor(so3.omega_edges, device=dev)
            self.z_rot = self.z_trans = self.noise_keys = None
            if keys is not None:
                self.noise_keys = noise_mod.keys_tensor(keys, dev)
            else:
                if noise_tape is None:
                    noise_tape = draw_noise_tape(diffuser, n_noisy, B, N)
                self.z_rot = torch.as_tensor(np.ascontiguousarray(noise_tape[0], dtype=np.float64), device=dev)
                self.z_trans = torch.as_tensor(np.ascontiguousarray(noise_tape[1], dtype=np.float64), device=dev)
            self.sc_ca = f32(data_init["sc_ca_t"])
            self.kept_steps, n_rows = steps, len(steps)
            self.frame_rows = self.kept_rigids = None
            self._row_of = None
            if self.kept:
                # step -> row of the kept arrays (-1: the step keeps no frame); the state is a two-row ring: x_t of step k = row k & 1
                rows = np.full(num_t, -1, dtype=np.int32)
                rows[steps] = np.arange(n_rows, dtype=np.int32)
                self._row_of = rows
                self.frame_rows = torch.as_tensor(rows, device=dev)
                self.rigid_traj = torch.empty(2, B, N, 7, device=dev)
                self.kept_rigids = torch.empty(n_rows, B, N, 7, device=dev) if aux_traj else None  # x_{t-1} of the kept steps
            else:
                self.rigid_traj = torch.empty(num_t + 1, B, N, 7, device=dev)  # row k = x_t of step k (row 0 = x_T), row k + 1 = its x_{t-1}
            self.rigid_traj[0] = rig0.to(device=dev, dtype=torch.float32)
            self.prot_traj = torch.empty(n_rows, B, N, 37, 3, device=dev)
            self.bb0_traj = torch.empty(n_rows, B, N, 37, 3, device=dev) if aux_traj else None
            self.trans_traj = torch.empty(n_rows, B, N, 3, device=dev) if aux_traj else None
            self.cursor = torch.zeros(2, dtype=torch.int32, device=dev)  # FdiptForwardArgs.step_cursor: {step index, ticket}
        # step graph: needs the noise rows of step k at row k (any tape drawn for this schedule), and at least a few steps to pay for capture
        # (device noise has no rows: the kernel draws step k's values from the cursor)
        self.graph = bool(graph) and n_noisy >= 3 and (keys is not None or (self.z_rot.shape[0] >= n_noisy and self.z_trans.shape[0] >= n_noisy))
        self._cursor_host = 0      # host mirror of cursor[0] (every writer of the cursor is ordered on this loop's stream)
        self._g1 = self._gn = None  # captured one-step / GRAPH_CHUNK-step graphs
        self.capture_seconds = 0.0
        self.captures = 0          # step graphs captured by this loop so far (a reset() loop replays them: the count stays)

    @property
    def rigids_t(self):
        """x_t of the next step to run (the row of the rigid trajectory the last finished step wrote)."""
        return self._x(self._next)

    _next = 0

    def _x(self, k):
        """Row of the state that holds x_t of step k (k = num_t: the final sample)."""
        return self.rigid_traj[k & 1] if self.kept else self.rigid_traj[k]

    def _row(self, k):
        """Row of the trajectory arrays that step k writes; None = the step keeps no frame."""
        if not self.kept:
            return k
        r = int(self._row_of[k])
        return None if r < 0 else r

    # ------------------------------------------------------------------ eager launches (pointers of step k on the host side)
    def _fwd(self, k, want_atoms, sc_update):
        # the forward itself hands the predicted CA positions to the next step's self-conditioning input (read at its start,
        # written at its end: no copy kernel)
        row = self._row(k)
        want_atoms = want_atoms and row is not None  # (a step that keeps no frame builds no rigid_0_traj row)
        direct = want_atoms and self.bb0_from_forward
        self.st.score_table = None if self.tab_all is None else self.tab_all[k]
        self.st.omega_edges = self.omega_edges
        self.st.forward(self._x(k), self.res_mask, self.fixed, self.sc_ca, self.net_aatype, self.gt_psi, self.t_all[k],
                        self.temb_all[k], self.sig_all[k], direct, ca_out=self.sc_ca if sc_update else None,
                        atom37_out=self.bb0_traj[row] if direct else None)  # rigid_0_traj row: straight into its slot
        if want_atoms and not direct:
            _backbone(self.model, self.B * self.N, self.st.rigids, None, None, self.st.psi, self.aatype, self.bb0_traj[row])

    def prime(self):
        """Self-conditioning priming call (utils.py:571-578)."""
        if self.embed_sc and self.self_condition:
            with torch.cuda.device(self.dev):
                self._fwd(0, False, True)

    def _verify_forward(self, k):
        """verify=n: the forward of step k runs twice on the same inputs (the first time without its side effects: no self-conditioning
        hand-over, no trajectory row) and every output must come back bit-identical — cheap insurance against silent corruption by a
        foreign process on the GPU.  One host synchronisation per verified step."""
        st = self.st
        self.st.score_table = None if self.tab_all is None else self.tab_all[k]
        self.st.omega_edges = self.omega_edges
        st.forward(self._x(k), self.res_mask, self.fixed, self.sc_ca, self.net_aatype, self.gt_psi, self.t_all[k],
                   self.temb_all[k], self.sig_all[k], False)
        return [x.clone() for x in (st.rigids, st.psi, st.rot_score, st.trans_score)]

    def _step_eager(self, k):
        st, t, n = self.st, self.reverse_steps[k], self.B * self.N
        first = self._verify_forward(k) if self.verify and k % self.verify == 0 else None
        self._fwd(k, self.aux_traj, self.embed_sc and t > self.min_t)
        if first is not None:
            for name, a, b in zip(("rigids", "psi", "rot_score", "trans_score"), first, (st.rigids, st.psi, st.rot_score, st.trans_score)):
                if not torch.equal(a, b):
                    raise _lib.FdiptError(f"verify: two runs of the forward of step {k} differ in `{name}` (max |diff| "
                                          f"{float((a - b).abs().max()):.3e}): results on this GPU are not reproducible — is another "
                                          "compute process using it? (DESIGN.md section 6)")
            self.verified += 1
        nxt, row = self._x(k + 1), self._row(k)
        if t > self.min_t:
            # x_{t-1} lands in its trajectory slot, which is the next forward's input; its atom37 frame comes out of the
            # same launch
            dev_noise = self.noise_keys is not None
            self.diffuser.reverse_device(self._x(k), st.rot_score, st.trans_score, self.diffuse_mask,
                                         None if dev_noise else self.z_rot[k], None if dev_noise else self.z_trans[k], t, self.dt,
                                         self.center, self.noise_scale, rigids_out=nxt, noise_keys=self.noise_keys, step=k,
                                         atoms=(st.psi, self.aatype, self.model.bb_tables, self.prot_traj[row]) if row is not None else None,
                                         traj=(st.rigids, self.fixed_mask, self.trans_traj[row]) if self.aux_traj and row is not None else None)
        else:  # last step: take the x_0 prediction, utils.py:373-374 (always a kept step)
            nxt.copy_(st.rigids)
            _backbone(self.model, n, nxt, None, None, st.psi, self.aatype, self.prot_traj[row])
            if self.aux_traj:  # (on the other steps the reverse-step launch writes this row)
                self.trans_traj[row] = self.diffuse_mask[..., None] * st.rigids[..., 4:] + self.fixed_mask[..., None] * nxt[..., 4:]
        if self.kept_rigids is not None and row is not None:  # (the cursor-addressed launch writes this row itself)
            self.kept_rigids[row].copy_(nxt)

    # ------------------------------------------------------------------ cursor-addressed launches (the same for every noisy step)
    def _enqueue_indexed(self):
        """One noisy step (forward, rigid_0_traj row, fused reverse step) on the rows ``cursor[0]`` of the trajectory arrays; the
        reverse-step launch advances the cursor.  Nothing here depends on the step: this is what the step graphs hold."""
        lib, st, d = _lib.load(), self.st, self.diffuser
        direct = self.aux_traj and self.bb0_from_forward
        st.score_table, st.omega_edges = self.tab_all, self.omega_edges
        st.forward(self.rigid_traj, self.res_mask, self.fixed, self.sc_ca, self.net_aatype, self.gt_psi, self.t_all, self.temb_all,
                   self.sig_all, direct, ca_out=self.sc_ca if self.embed_sc else None, atom37_out=self.bb0_traj if direct else None,
                   step_cursor=self.cursor, frame_rows=self.frame_rows, state_ring=self.kept)
        if self.aux_traj and not direct:  # (the kept entry is the indexed one with the row map behind the cursor)
            args = [self.B * self.N, _lib.ptr(st.rigids), _lib.ptr(st.psi), _lib.ptr(self.aatype), _lib.ptr(self.model.bb_tables),
                    _lib.ptr(self.bb0_traj), _lib.ptr(self.cursor)]
            if self.kept:
                _lib.check(lib.fdipt_backbone_atoms_kept(*args, _lib.ptr(self.frame_rows), _lib.stream_ptr()), "backbone_atoms_kept")
            else:
                _lib.check(lib.fdipt_backbone_atoms_indexed(*args, _lib.stream_ptr()), "backbone_atoms_indexed")
        so3, r3 = d._so3_diffuser, d._r3_diffuser
        a = _lib.ReverseIndexed()
        a.B, a.N = self.B, self.N
        for name, tns in (("rigid_traj", self.rigid_traj), ("rot_score", st.rot_score), ("trans_score", st.trans_score),
                          ("diffuse_mask", self.diffuse_mask), ("z_rot", self.z_rot), ("z_trans", self.z_trans), ("t_table", self.t_tab),
                          ("psi", st.psi), ("aatype", self.aatype), ("bb_tables", self.model.bb_tables), ("prot_traj", self.prot_traj),
                          ("pred_rigids", st.rigids if self.aux_traj else None), ("traj_fixed_mask", self.fixed_mask if self.aux_traj else None),
                          ("trans_traj", self.trans_traj), ("step_cursor", self.cursor), ("frame_rows", self.frame_rows),
                          ("kept_rigids", self.kept_rigids)):
            setattr(a, name, _lib.ptr(tns))
        a.state_ring = int(self.kept)
        a.dt, a.noise_scale = float(self.dt), float(self.noise_scale)
        a.center, a.diffuse_rot, a.diffuse_trans = int(bool(self.center)), int(bool(d._diffuse_rot)), int(bool(d._diffuse_trans))
        a.so3_min_sigma, a.so3_max_sigma, a.r3_min_b, a.r3_max_b = so3.min_sigma, so3.max_sigma, r3.min_b, r3.max_b
        a.coordinate_scaling = r3._r3_conf.coordinate_scaling
        if self.noise_keys is not None:  # (z_rot / z_trans are NULL: the draws of step cursor[0])
            _lib.check(lib.fdipt_se3_reverse_step_indexed_gen(C.byref(a), _lib.ptr(self.noise_keys), _lib.stream_ptr()),
                       "se3_reverse_step_indexed_gen")
        else:
            _lib.check(lib.fdipt_se3_reverse_step_indexed(C.byref(a), _lib.stream_ptr()), "se3_reverse_step_indexed")

    def capture_step_graph(self, n_steps=1):
        """A HIP graph of ``n_steps`` consecutive cursor-addressed steps (nothing runs; whatever ``self.st`` carries — event pairs,
        the clock probe — is captured with it).  Capture happens on a side stream: the caller's stream may be the null stream."""
        import time
        t0 = time.perf_counter()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=self.dev)
        with torch.cuda.stream(side):
            g.capture_begin(capture_error_mode="thread_local")
            try:
                for _ in range(n_steps):
                    self._enqueue_indexed()
            finally:
                g.capture_end()
        self.capture_seconds += time.perf_counter() - t0
        self.captures += 1
        self._captured_weights = getattr(self.model, "weights_version", 0)  # the graphs bake the weight / derived-buffer pointers in
        return g

    def _set_cursor(self, k):
        if self._cursor_host != k:
            self.cursor[:1].fill_(k)
            self._cursor_host = k

    # (device, precision, kernel flags, B, N) of the cursor-addressed steps that have run in this process: the kernels' lazy per-device
    # set-up (raised dynamic-LDS caps) must not fall into a capture, so the first such step of a shape class is enqueued eagerly
    _WARM: set = set()

    def _warm_key(self):
        # every field of FdiptDims (widths select the fused or the generic kernels) and the options that change which kernels a step
        # launches (round-5 advisor: a second model with other widths at the same B, N was treated as warm)
        return (str(self.dev), bytes(self.model.dims), self.B, self.N, bool(self.aux_traj), bool(self.bb0_from_forward),
                bool(self._inpainting), self.tab_all is not None, bool(self.embed_sc), bool(self.self_condition),
                self.noise_keys is not None, bool(self.kept))

    def prepare(self):
        """Capture the step graphs now (otherwise: lazily at the first replay).  Nothing runs on the GPU."""
        if self.graph and self._warm_key() in self._WARM:
            with torch.cuda.device(self.dev):
                if self._g1 is None:
                    self._g1 = self.capture_step_graph(1)
                if self._gn is None and self.GRAPH_CHUNK > 1 and self.n_noisy >= 2 * self.GRAPH_CHUNK:
                    self._gn = self.capture_step_graph(self.GRAPH_CHUNK)
        return self

    def _advance(self, k, n, eager=False):
        """Steps k .. k+n-1 (all noisy) through the cursor: launch by launch the first time a shape class runs in the process (or with
        ``eager``: bench.py's event-bracketed steps — events recorded inside a graph cannot be timed on ROCm), graph replays otherwise."""
        self._set_cursor(k)
        if (self._g1 is not None or self._gn is not None) and self._captured_weights != getattr(self.model, "weights_version", 0):
            self._g1 = self._gn = None  # the model's weights were (re)loaded behind this loop: its captured graphs point at freed buffers
        if eager or self._warm_key() not in self._WARM:
            for _ in range(n):
                self._enqueue_indexed()
            self._WARM.add(self._warm_key())
        elif n > 1 and n == self.GRAPH_CHUNK:
            if self._gn is None:
                self._gn = self.capture_step_graph(n)
            self._gn.replay()
        else:
            if self._g1 is None:
                self._g1 = self.capture_step_graph(1)
            for _ in range(n):
                self._g1.replay()
        self._cursor_host = k + n

    def step(self, k, eager=False):
        """one_step_inference (utils.py:292-412) for reverse step k."""
        with torch.cuda.device(self.dev):
            if self.graph and k < self.n_noisy and not (self.verify and k % self.verify == 0):
                self._advance(k, 1, eager)
            else:
                self._step_eager(k)
        self._next = k + 1

    def run_steps(self, k_begin, k_end, eager_steps=(), before_step=None):
        """Steps k_begin .. k_end - 1 in sequence (graph replays, ``GRAPH_CHUNK`` steps at a time where that many noisy steps remain).
        ``eager_steps``: steps to enqueue launch by launch instead, ``before_step(k)`` called ahead of each of them and ``before_step(None)``
        behind it (bench.py: HIP events around the dominant kernel's launches of a few steps)."""
        k, eager_steps = k_begin, set(eager_steps)
        while k < k_end:
            n = self.GRAPH_CHUNK
            if (not self.graph or n < 2 or min(self.n_noisy, k_end) - k < n or self._warm_key() not in self._WARM
                    or any(kk in eager_steps or (self.verify and kk % self.verify == 0) for kk in range(k, k + n))):
                n = 1
            if n == 1:
                if k in eager_steps and before_step is not None:
                    before_step(k)
                self.step(k, eager=k in eager_steps)
                if k in eager_steps and before_step is not None:
                    before_step(None)
            else:
                with torch.cuda.device(self.dev):
                    self._advance(k, n)
            k += n
        self._next = k_end
        return self

    def run(self, eager_steps=(), before_step=None):
        """The whole trajectory: priming forward, then every step."""
        self.prime()
        return self.run_steps(0, self.num_t, eager_steps, before_step)

    def results(self, return_device=False):
        st = self.st
        psi_pred = st.psi.to(self.gt_tors.dtype).clone() if self.gt_tors.dtype == torch.float64 else st.psi.clone()
        conv = (lambda x: torch.flip(x, (0,))) if return_device else (lambda x: np.flip(x.cpu().numpy(), (0,)))
        ret = {"prot_traj": conv(self.prot_traj)}
        if self.kept:  # the kept k values in the arrays' (flipped) order: row 0 = the final step
            ret["kept_steps"] = self.kept_steps[::-1].copy()
        if self.aux_traj:
            ret["rigid_traj"] = conv(self.kept_rigids if self.kept else self.rigid_traj)  # (kept: x_{t-1} of the kept steps, no x_T row)
            ret["trans_traj"] = conv(self.trans_traj)
            ret["psi_pred"] = psi_pred[None]
            ret["rigid_0_traj"] = conv(self.bb0_traj)
        return ret

    def reset(self, data_init, noise_tape=None, noise_keys=None):
        """Load another batch of the same (B, N, num_t, min_t, options) into this loop's device buffers and rewind it: x_T, the masks,
        ``sc_ca``, the aatype views, ``gt_psi``, the noise tape (drawn from ``np.random`` when not given, as at construction) or keys, what
        the ``BatchState`` derives from ``seq_idx``, and the cursor are overwritten IN PLACE — the captured step graphs hold these
        pointers and are replayed as they are.  Whatever would change the launch sequence raises ``ValueError`` instead (another
        ``_warm_key()``: a switch of ``bb0_from_forward``, of an aatype view between present and absent, of the score table).  Work of the
        previous trajectory that is still in flight must be on the current stream (``results()`` copies are)."""
        dev = self.dev
        gpu_guard.check(dev, what="inference_fn")
        rig0 = data_init["rigids_t"]
        _lib.require_cuda(rig0, "inference_fn")
        if tuple(rig0.shape[:2]) != (self.B, self.N):
            raise ValueError(f"reset: the loop holds buffers and graphs for B, N = {self.B}, {self.N}; got {tuple(rig0.shape[:2])}")
        if (noise_keys is not None) != (self.noise_keys is not None):
            raise ValueError("reset: the noise mode (host tape / device keys) is part of the captured launch sequence")
        if self.diffuser._so3_diffuser.use_cached_score != (self.tab_all is not None):
            raise ValueError("reset: so3.use_cached_score changed behind the loop: the score-table switch selects other launches")
        before = self._warm_key()
        with torch.cuda.device(dev):
            f32 = lambda x: x.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
            fixed = f32(data_init["fixed_mask"])
            aatype, net_aatype, same = _aatype_views(self.model, data_init, fixed, self._inpainting, self._input_aatype, dev)
            if same != self.bb0_from_forward or (aatype is None) != (self.aatype is None) or (net_aatype is None) != (self.net_aatype is None):
                raise ValueError("reset: this batch changes who builds the rigid_0_traj rows (bb0_from_forward / the aatype views): the captured "
                                 "launch sequence does not fit it; construct a new loop")
            seq_idx = data_init["seq_idx"]
            if tuple(seq_idx.shape) != (self.B, self.N):
                raise ValueError(f"reset: seq_idx of shape {tuple(seq_idx.shape)}, the loop holds B, N = {self.B}, {self.N}")
            keys = tape = None
            if self.noise_keys is not None:
                keys = noise_mod.keys_tensor(noise_mod.resolve("device", noise_keys, noise_tape, self.B), dev)
            else:
                if noise_tape is None:
                    noise_tape = draw_noise_tape(self.diffuser, self.n_noisy, self.B, self.N)
                tape = [torch.as_tensor(np.ascontiguousarray(z, dtype=np.float64)) for z in noise_tape]
                for dst, z in zip((self.z_rot, self.z_trans), tape):
                    if tuple(z.shape) != tuple(dst.shape):
                        raise ValueError(f"reset: noise tape of shape {tuple(z.shape)}, the loop's is {tuple(dst.shape)}")
            # ---- every check has passed: from here on the loop's buffers are overwritten
            if getattr(self.model, "_state", None) is self.st:
                # a loop built without state= shares the model's cached BatchState, which refresh() rewrites in place: the loop takes it
                # over (its graphs hold its pointers) and the model builds a new one for its next caller
                self.model._state = self.model._state_key = None
            if keys is not None:
                self.noise_keys.copy_(keys)
            else:
                self.z_rot.copy_(tape[0])
                self.z_trans.copy_(tape[1])
            self.res_mask.copy_(f32(data_init["res_mask"]))
            self.fixed.copy_(fixed)
            torch.mul(self.fixed, self.res_mask, out=self.fixed_mask)
            torch.mul(1 - self.fixed, self.res_mask, out=self.diffuse_mask)
            if aatype is not None:
                self.aatype.copy_(aatype)
            if net_aatype is not None:
                self.net_aatype.copy_(net_aatype)
            self.gt_tors = data_init["torsion_angles_sin_cos"]
            self.gt_psi.copy_(f32(self.gt_tors[..., 2, :]))
            self.sc_ca.copy_(f32(data_init["sc_ca_t"]))
            self.rigid_traj[0].copy_(rig0.to(device=dev, dtype=torch.float32))
            if not self.st.refresh(seq_idx):
                self._g1 = self._gn = None  # the relative-position range changed: new set-up table and launch scalars, captured again
            self.cursor.zero_()
        self._cursor_host, self._next, self.verified = 0, 0, 0
        assert self._warm_key() == before  # (every field of the key is either constant or checked above)
        return self


class Session:
    """Loops (buffers + captured step graphs) kept between ``inference_fn(..., session=sess)`` calls: a call whose model, shape, schedule
    and options match an earlier one ``reset()``s that loop and replays its graphs instead of allocating and capturing again.  Keyed by
    model identity (and its weights version) + what ``ReverseLoop._warm_key()`` covers + (num_t, min_t, keep, noise mode) and the scalar
    options.  At most ``max_loops`` loops stay alive (least recently used goes first), so a sweep over lengths does not pin HBM;
    ``close()`` drops them all.  One session per process and device stream: calls must not overlap."""

    def __init__(self, max_loops: int = 4):
        from collections import OrderedDict
        if max_loops < 1:
            raise ValueError("max_loops must be >= 1")
        self.max_loops, self.loops = int(max_loops), OrderedDict()
        self.hits = self.misses = 0

    def loop(self, model, diffuser, data_init, num_t, min_t, noise_tape=None, noise_keys=None, **opts):
        """A loop loaded with ``data_init`` and rewound: an earlier one (``reset``) or a new one.  ``opts``: ``ReverseLoop``'s keyword options."""
        dev = model.device
        version = getattr(model, "weights_version", 0)
        for k in [k for k in self.loops if k[0] == id(model) and k[1] != version]:
            del self.loops[k]  # loops of this model from before a weight reload can never hit again: free them now
        fixed = data_init["fixed_mask"].to(device=dev, dtype=torch.float32)
        same = _aatype_views(model, data_init, fixed, opts.get("inpainting", False), opts.get("input_aatype", False), dev)[2]
        B, N = (int(x) for x in data_init["rigids_t"].shape[:2])
        # (id() is a safe identity here because a cached loop holds references to its model and diffuser: neither id can be reused by
        #  another object while the entry lives)
        key = (id(model), version, id(diffuser), str(dev), bytes(model.dims), B, N, int(num_t), float(min_t),
               noise_keys is not None, same, data_init.get("aatype") is None, bool(diffuser._so3_diffuser.use_cached_score),
               tuple(sorted((k, v if isinstance(v, (str, int, float, bool, type(None))) else repr(v)) for k, v in opts.items())))
        lp = self.loops.get(key)
        if lp is not None:
            lp.reset(data_init, noise_tape=noise_tape, noise_keys=noise_keys)  # (raises before it writes: the loop stays cached and usable)
            self.hits += 1
            self.loops.move_to_end(key)
            return lp
        else:
            self.misses += 1
            while len(self.loops) >= self.max_loops:
                self.loops.popitem(last=False)
            # a batch state of the loop's own: reset() rewrites it in place, which must not happen to the model's cached one
            how = dict(noise="device", noise_keys=noise_keys) if noise_keys is not None else dict(noise_tape=noise_tape)
            lp = ReverseLoop(model, diffuser, data_init, num_t, min_t, state=model.new_batch_state(data_init["seq_idx"]), **how, **opts)
        self.loops[key] = lp
        return lp

    def close(self):
        self.loops.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


_SUB_BATCH_STREAMS: dict = {}  # device -> HIP streams of the sub-batches, created once (HIP multiplexes streams onto a few hardware
                               # queues: fresh streams per trajectory would end up sharing one)


def _sub_batch_streams(dev, n):
    pool = _SUB_BATCH_STREAMS.setdefault(str(dev), [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


class StreamedLoops:
    """The batch cut into ``n_streams`` sub-batches, each a ``ReverseLoop`` with its own workspace on its own HIP stream.

    The node path of the score network (M = B*N rows: a few dozen workgroups per launch) is latency-bound and leaves most of the
    256 CUs idle, while the pair path (EdgeTransition, IPA attention, o_pair) is throughput-bound: with two sub-batches in
    flight the GPU runs one sub-batch's pair kernels under the other's node-path launches.  Results do not change: a sample's
    trajectory is bit-identical whatever batch it rides in (tests: test_batch_of_equal_samples_matches_single,
    test_concurrent_forwards_are_bit_identical).  Same interface as ``ReverseLoop`` (prime / step / results)."""

    MAX_STREAMS = 2   # experimental feature, verified for two streams only (see below)
    MAX_LENGTH = 384  # ... and for N <= 384 only
    OPT_IN_ENV = "FDIPT_EXPERIMENTAL_STREAMS"  # more than one stream is an explicit opt-in: experimental=True or this variable set to 1

    def __init__(self, model, diffuser, data_init, n_streams, num_t, min_t, noise_tape=None, reserve_cus=48, experimental=False,
                 noise="host", noise_keys=None, **kw):
        # Soak results (tools/soak_streams.sh, tools/streams_stat.py; trajectories against the single-stream run):
        #   * N = 128 / 300, two streams, any number of reserved CUs: 0 mismatching runs of ~400;
        #   * N = 300, three or four streams: 15 - 40 % of the runs differ in one sample from some step on;
        #   * N = 512 / 724 / 1000, two streams: 1 / 12, 3 / 12, up to 11 / 12 mismatching runs depending on `reserve_cus`.
        # Cause (round 4): on these GPUs a wave that runs a half-precision MFMA and lane-masked VALU code disturbs OTHER
        # waves on its SIMD (their last 16-lane pass is written with the foreign EXEC mask) — reproduced without library code by
        # tools/micro/hazard_repro.hip.  It needs waves of different kernels on one SIMD, which only concurrent streams / processes
        # produce; inside the verified range the kernels' footprints happen to keep the small fp64 kernels off the attention's SIMDs.
        # Nothing in software removes it, so: an explicit opt-in, refused beyond the range the soaks cover.  The single-stream path
        # is not exposed and is bit-reproducible at every size.
        import os
        B = data_init["rigids_t"].shape[0]
        keys = noise_mod.resolve(noise, noise_keys, noise_tape, int(B))
        requested, n_streams = n_streams, max(1, min(n_streams, B))  # (the limits apply to what would actually run)
        if n_streams > self.MAX_STREAMS:
            raise ValueError(f"streams={requested}: sub-batch streams are verified bit-identical to the single-stream run for at most "
                             f"{self.MAX_STREAMS} streams")
        if n_streams > 1 and data_init["rigids_t"].shape[1] > self.MAX_LENGTH:
            raise ValueError(f"streams={requested} at N = {data_init['rigids_t'].shape[1]}: sub-batch streams are verified bit-identical to "
                             f"the single-stream run for N <= {self.MAX_LENGTH} only")
        if n_streams > 1 and not (experimental or os.environ.get(self.OPT_IN_ENV) == "1"):
            raise ValueError(f"streams={requested}: concurrent sub-batch streams are an experimental feature with an open correctness item beyond "
                             f"the verified range (DESIGN.md, concurrency): opt in with experimental_streams=True or {self.OPT_IN_ENV}=1")
        cuts = [round(i * B / n_streams) for i in range(n_streams + 1)]
        self.dev = model.device
        if noise_tape is None and keys is None:
            n_noisy = int(np.sum(np.linspace(min_t, 1.0, num_t)[::-1] > min_t))
            noise_tape = draw_noise_tape(diffuser, n_noisy, B, data_init["rigids_t"].shape[1])
        self.loops, self.streams = [], _sub_batch_streams(self.dev, n_streams)
        with torch.cuda.device(self.dev):
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                sub = {k: v[lo:hi] for k, v in data_init.items() if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B}
                st = model.new_batch_state(sub["seq_idx"])
                st.reserve_cus = reserve_cus if n_streams > 1 else 0  # the persistent pair kernels leave CUs to the other streams
                # (each sub-batch takes its slice of the tape, or of the keys: a sample's draws do not depend on the batch it rides in)
                sub_noise = dict(noise="device", noise_keys=keys[lo:hi]) if keys is not None else dict(
                    noise_tape=tuple(z[:, lo:hi] for z in noise_tape))
                self.loops.append(ReverseLoop(model, diffuser, sub, num_t, min_t, state=st, graph=False, **sub_noise, **kw))
        torch.cuda.synchronize(self.dev)  # set-up ran on the current stream
        self.st = self.loops[0].st

    def __del__(self):
        # the loops' buffers were allocated on the caller's stream and are used on the side streams: if the object is dropped
        # early (an exception mid-trajectory) the caching allocator must not hand them out while side-stream kernels still run
        try:
            self.synchronize()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass

    def _each(self, fn):
        # (no per-step ordering against the caller's stream: an event on the default stream orders every sub-batch stream behind
        #  all work enqueued before it, i.e. the sub-batches would run one after the other; set-up was synchronised once)
        for loop, s in zip(self.loops, self.streams):
            with torch.cuda.stream(s):
                fn(loop)

    def prime(self):
        self._each(lambda lp: lp.prime())

    def step(self, k):
        self._each(lambda lp: lp.step(k))

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def results(self, return_device=False):
        self.synchronize()
        parts = [lp.results(return_device) for lp in self.loops]
        cat = lambda xs: torch.cat(xs, 1) if torch.is_tensor(xs[0]) else np.concatenate(xs, 1)  # noqa: E731
        # (every returned array carries the batch on axis 1; kept_steps has none)
        return {k: parts[0][k] if k == "kept_steps" else cat([p[k] for p in parts]) for k in parts[0]}


def inference_fn(model, diffuser, data_init, num_t, min_t, center=True, aux_traj=False, self_condition=True,
                 noise_scale=1.0, embed_self_conditioning=True, inpainting=False, input_aatype=False, noise_tape=None,
                 return_device=False, streams=1, experimental_streams=False, graph=True, verify=0, pad_to_four=True,
                 noise="host", noise_keys=None, keep="all", session=None):
    """Same arguments / returned keys as the reference.  ``noise_tape=(z_rot, z_trans)`` ([num_t-1,B,N,3] float64
    N(0,1) draws) overrides the global ``np.random`` stream (sample-sharded runs).  ``data_init`` tensors carry a
    leading batch dimension B >= 1 (the reference always passes B = 1).  ``graph=True`` (default): the steps are replays of a HIP
    graph captured once per trajectory (``ReverseLoop``: same kernels and bits, ~1/70 of the host work); ``graph=False``: every step
    enqueued launch by launch.  ``verify=k``: the forward of every k-th step runs twice and must reproduce its bits (``FdiptError``
    otherwise; one host sync per verified step) — for GPUs shared with other compute processes (``gpu_guard``).  ``streams=n``: the batch runs as n sub-batches on n HIP streams (same results; the latency-bound
    node path of one sub-batch overlaps the pair kernels of the other) — experimental: needs ``experimental_streams=True`` (or
    FDIPT_EXPERIMENTAL_STREAMS=1), at most two streams, N <= 384 (``StreamedLoops``; eager launches).  ``noise="device"`` (opt-in; the
    default ``"host"`` is the reference's stream): no tape is drawn or uploaded, the reverse-step kernel draws its N(0,1) values from
    ``noise_keys`` (B 64-bit keys as a sequence / int64 tensor; an int ``s`` means ``s, s + 1, ...``) — a draw depends on (key, step,
    residue, component) only, ``noise.filled_tape`` gives the tape that reproduces the run bit for bit.  ``keep="last"`` / ``keep=s``
    (opt-in; ``"all"`` is the reference's full trajectories): only the frames of the steps ``kept_steps(num_t, keep)`` are built, held
    and returned — the returned arrays (``rigid_traj`` too: x_{t-1} of the kept steps, no x_T row) share the leading length
    ``len(kept_steps)``, row 0 the sample, bit-identical to rows ``[::s]`` of the ``"all"`` run, and ``kept_steps`` names their steps.
    ``session=inference.Session()``: the loop's buffers and captured graphs are kept and reused by the next call of the same shape and
    options (``ReverseLoop.reset``); the returned arrays never alias them.  Not with ``streams > 1``."""
    kept_steps(num_t, keep)
    if session is not None and streams > 1:
        raise ValueError("session= keeps single-stream loops: it cannot be combined with streams > 1")
    keys = noise_mod.resolve(noise, noise_keys, noise_tape, int(data_init["rigids_t"].shape[0]))
    # Round 6: lengths that are no multiple of 4 run the half-precision mode's fall-back pair kernels (edge_transition3, the pass over z for
    # o_pair): 2.94 ms per step at N = 302 against 2.14 at 304 (eight samples).  ``pad_to_four`` (default) pads such a sample with masked rows
    # (res_mask = 0, identity frames, zero noise: sharding.pad_item, what run_sharded does to mixed-length batches) and cuts the returned
    # arrays back to N — the real residues see the same arithmetic as in a run_sharded batch of their kernel class.  The noise tape is drawn
    # for the REAL residues first (the reference's np.random order is untouched).
    n_real = int(data_init["rigids_t"].shape[1])
    n_pad = -(-n_real // 4) * 4
    padded = bool(pad_to_four) and n_pad != n_real and getattr(model, "precision", _lib.PREC_F32) != _lib.PREC_F32
    if padded:
        from . import sharding
        # Device noise needs no change of values here: padding rows are not diffused (diffuse_mask = 0 multiplies their perturbation) and
        # real rows keep their residue index, which — not the padded length — is what a draw depends on.
        if noise_tape is None and keys is None:
            n_noisy = int(np.sum(np.linspace(min_t, 1.0, num_t)[::-1] > min_t))
            noise_tape = draw_noise_tape(diffuser, n_noisy, int(data_init["rigids_t"].shape[0]), n_real)
        data_init, noise_tape = sharding.pad_item(data_init, noise_tape, n_pad)
    if streams > 1 and data_init["rigids_t"].shape[0] > 1:  # sub-batches on their own HIP streams (same results)
        # (the sub-loops are eager ReverseLoops: verify= is passed through to them, graph= does not apply)
        loop = StreamedLoops(model, diffuser, data_init, streams, num_t, min_t, noise_tape=noise_tape, center=center, aux_traj=aux_traj,
                             self_condition=self_condition, noise_scale=noise_scale, embed_self_conditioning=embed_self_conditioning,
                             inpainting=inpainting, input_aatype=input_aatype, experimental=experimental_streams, verify=verify,
                             noise=noise, noise_keys=keys, keep=keep)
        loop.prime()
        for k in range(num_t):
            loop.step(k)
    elif session is not None:
        loop = session.loop(model, diffuser, data_init, num_t, min_t, noise_tape=noise_tape, noise_keys=keys, center=center,
                            aux_traj=aux_traj, self_condition=self_condition, noise_scale=noise_scale,
                            embed_self_conditioning=embed_self_conditioning, inpainting=inpainting, input_aatype=input_aatype,
                            graph=graph, verify=verify, keep=keep).run()
    else:
        loop = ReverseLoop(model, diffuser, data_init, num_t, min_t, center, aux_traj, self_condition, noise_scale,
                           embed_self_conditioning, inpainting, input_aatype, noise_tape, graph=graph, verify=verify, noise=noise,
                           noise_keys=keys, keep=keep).run()
    res = loop.results(return_device)
    if padded:  # (every returned array carries the residues on the axis behind the batch; kept_steps has neither)
        res = {k: v if k == "kept_steps" else v[:, :, :n_real] for k, v in res.items()}
    return res
