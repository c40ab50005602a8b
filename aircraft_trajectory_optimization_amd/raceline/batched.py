'''
Batched evaluation of a raceline NLP on one HIP device.

B independent instances share one ProblemSpec (same track, N, K, model). Decision
vectors, constraints, Jacobian values and gradients live in HBM as torch tensors in the
library's INTERLEAVED layout ([element][instance]); evaluation is a single libato call
(ato_eval) on the current torch stream. This is the drop-in for the reference's per-
iterate nlp_g / nlp_jac_g / nlp_f / nlp_grad_f calls (base_raceline.py:165, via IPOPT).
'''
from typing import Optional, Tuple

import numpy as np
import torch

from aircraft_trajectory_optimization_amd import native
from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec


class BatchedNLP:
    ''' device-resident batch of NLP instances '''

    def __init__(self, spec: ProblemSpec, batch: int, dtype: torch.dtype = torch.float64,
                 layout: int = native.ATO_LAYOUT_INTERLEAVED, device: Optional[torch.device] = None,
                 buffers: bool = True):
        if not torch.cuda.is_available():
            raise RuntimeError('BatchedNLP needs a HIP device (torch.cuda.is_available() is False)')
        self.device = device or torch.device('cuda', torch.cuda.current_device())
        with torch.cuda.device(self.device):
            self.problem = native.NativeProblem(spec.native_spec())
        self.spec = spec
        self.batch = int(batch)
        self.dtype = dtype
        self.layout = layout
        self.fp32 = dtype == torch.float32
        nw, ng, nnz, B = self.problem.nw, self.problem.ng, self.problem.nnz, self.batch
        shape = (lambda n: (n, B)) if layout == native.ATO_LAYOUT_INTERLEAVED else (lambda n: (B, n))
        opts = {'device': self.device, 'dtype': dtype}
        # resident input / output buffers of evaluate(); buffers=False: the caller passes its own
        # (the solver's evaluator, whose outputs are fresh tensors: at B = 8192 J alone is GBs)
        self.w = torch.zeros(shape(nw), **opts) if buffers else None
        self.g = torch.zeros(shape(ng), **opts) if buffers else None
        self.jac = torch.zeros(shape(nnz), **opts) if buffers else None
        self.grad_f = torch.zeros(shape(nw), **opts) if buffers else None
        self.f = torch.zeros(B, **opts) if buffers else None
        self.problem.reserve(B)
        # evaluations write only the structural nonzeros of grad f (its other entries stay the zeros of
        # the buffers above; the solver's fresh output tensors are zero-filled, solver/batched_ipm.py)
        self.problem.gradf_mode(True)
        self.row_ptr, self.col = self.problem.sparsity()
        self.lbg, self.ubg = self.problem.bounds()
        self.isph = None          # per-instance sphere centres [2 P][B] (set_instance_spheres)
        self._n_planes = None     # gates given to set_gates (None: the problem's own, len(spec.gates))

    def set_instance_spheres(self, tables: Optional[np.ndarray]):
        '''
        Per-instance obstacle tubes (config 4): tables (B, P, 3) of (dy, dn, available radius) per
        node, one ObstacleFreeTube.sphere_table per instance (mesh_obstacle.py:219-237). The centres go
        to the device ([2 P][B], read by the sphere rows); lbg / ubg become per-instance (ng, B) arrays
        with each instance's radius^2 in its sphere rows. None returns to the spec's shared table.
        '''
        if tables is None:
            self.isph = None
            self.lbg, self.ubg = self.problem.bounds()
            return
        if self.spec.sphere_table is None:
            raise ValueError('per-instance spheres need a problem with sphere rows (spec.sphere_table)')
        P = self.spec.P
        T = np.asarray(tables, np.float64).reshape(self.batch, P, 3)
        cen = np.ascontiguousarray(T[:, :, :2].reshape(self.batch, 2 * P).T)
        self.isph = torch.as_tensor(cen, device=self.device)
        rows = self.problem.sphere_rows(P)
        lb, ub = self.problem.bounds()
        self.lbg = np.repeat(lb[:, None], self.batch, axis=1)
        self.ubg = np.repeat(ub[:, None], self.batch, axis=1)
        has = rows >= 0
        self.ubg[rows[has], :] = (T[:, has, 2] ** 2).T
        self.sphere_rows = rows

    def _bind_spheres(self):
        ''' the handle may be shared (subset evaluators): point it at this batch's centres '''
        if self.spec.sphere_table is not None:
            self.problem.set_instance_spheres(self.isph.data_ptr() if self.isph is not None else 0, self.batch)

    @property
    def sizes(self) -> Tuple[int, int, int]:
        ''' nw, ng, nnz '''
        return self.problem.nw, self.problem.ng, self.problem.nnz

    def set_w(self, W: np.ndarray):
        ''' W: (B, nw) host array of decision vectors '''
        W = np.asarray(W, dtype=np.float64).reshape(self.batch, -1)
        t = torch.as_tensor(W, dtype=self.dtype)
        if self.layout == native.ATO_LAYOUT_INTERLEAVED:
            t = t.T.contiguous()
        self.w.copy_(t.to(self.device))

    def evaluate(self, g: bool = True, jac: bool = True, cost: bool = True, stream=None):
        ''' launch the evaluation (asynchronous on `stream`, default the current torch stream) '''
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._bind_spheres()
        self.problem.eval_ptrs(
            self.batch, self.w.data_ptr(),
            g=self.g.data_ptr() if g else 0,
            jac=self.jac.data_ptr() if jac else 0,
            f=self.f.data_ptr() if cost else 0,
            grad_f=self.grad_f.data_ptr() if cost else 0,
            layout=self.layout, stream=st.cuda_stream, fp32=self.fp32)

    def hessian(self, lam: torch.Tensor, sigma: torch.Tensor, stream=None) -> torch.Tensor:
        '''
        Hessian of the Lagrangian (lower triangle, values in hess_sparsity() order) for multipliers
        lam (same layout as g) and objective factors sigma [B]; fp64 only.
        '''
        if self.fp32:
            raise TypeError('the Hessian is evaluated in fp64')
        if not hasattr(self, 'hess_row_ptr'):
            self.hess_row_ptr, self.hess_col, self.hess_colors = self.problem.hess_sparsity()
            shape = (len(self.hess_col), self.batch) if self.layout == native.ATO_LAYOUT_INTERLEAVED \
                else (self.batch, len(self.hess_col))
            self.hess = torch.zeros(shape, device=self.device, dtype=torch.float64)
            self.problem.reserve(self.batch)
        lam = lam.contiguous()
        sigma = sigma.contiguous()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._bind_spheres()
        self.problem.hess_eval_ptrs(self.batch, self.w.data_ptr(), lam.data_ptr(), sigma.data_ptr(),
                                    self.hess.data_ptr(), layout=self.layout, stream=st.cuda_stream)
        return self.hess

    def _columns(self, W, what: str) -> torch.Tensor:
        ''' the decision vectors a post-solve check (`what`) reads, contiguous fp64 on the device in this batch's
        layout: None is the resident w, a host array (B, nw) is uploaded, a device tensor is checked '''
        B, il = self.batch, self.layout == native.ATO_LAYOUT_INTERLEAVED
        if W is None:
            if self.w is None or self.fp32:
                raise TypeError(f'{what} needs fp64 decision vectors (pass W)')
            W = self.w
        elif not torch.is_tensor(W):
            t = torch.as_tensor(np.array(W, np.float64).reshape(B, -1))
            W = (t.T.contiguous() if il else t.contiguous()).to(self.device)
        if W.dtype != torch.float64 or tuple(W.shape) != ((self.problem.nw, B) if il else (B, self.problem.nw)):
            raise ValueError('W must be fp64 in the layout of this batch')
        return W.contiguous()

    def _ensure_line(self):
        ''' the centreline table of a parametric problem, handed to the library once (clearance and audit) '''
        sp_ = self.spec
        if sp_.param and not getattr(self, '_clearance_line', False) and not sp_.rk4:
            self.problem.clearance_set_line(sp_.line_table())
            self._clearance_line = True

    def _sample_points(self, samples: int) -> int:
        ''' points per interval of clearance() and audit(): the library's clearance_points (csrc/ato_sample.hpp) '''
        return self.spec.K1 if samples == 0 else samples + 1

    def replay(self, W=None, substeps: int = 16, trajectory: bool = False, stream=None):
        '''
        Replay decision vectors through the vehicle ODE (ato_replay, asynchronous on `stream`): per
        interval the start state, lifted to the global model, is integrated over h_n with `substeps`
        RK4 steps under the solution's own inputs and compared with the collocation polynomial's end
        value. W: fp64 device tensor in this batch's layout ((nw, B) interleaved, (B, nw) instance-
        major) or a host array (B, nw); None: the resident w. Returns (zsim, err, traj) in the layout:
        interleaved (N, nz, B), (N, 4, B), (N, substeps, nz, B); instance-major (B, N, nz), (B, N, 4),
        (B, N, substeps, nz); traj is None unless `trajectory`. err rows: position (m), attitude (rad),
        velocity (m/s), body rate (rad/s). Problems the replay does not cover raise NotImplementedError.
        '''
        sp_, B = self.spec, self.batch
        il = self.layout == native.ATO_LAYOUT_INTERLEAVED
        W = self._columns(W, 'replay')
        if sp_.param and not getattr(self, '_replay_lift', False) and not sp_.rk4 and sp_.vehicle.global_r:
            self.problem.replay_set_lift(sp_.lift_table())
            self._replay_lift = True
        S = int(substeps)
        opts = {'device': self.device, 'dtype': torch.float64}
        shape = (lambda *d: (*d, B)) if il else (lambda *d: (B, *d))
        zsim = torch.empty(shape(sp_.N, sp_.nz), **opts)
        err = torch.empty(shape(sp_.N, 4), **opts)
        traj = torch.empty(shape(sp_.N, max(S, 1), sp_.nz), **opts) if trajectory else None
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.problem.replay_ptrs(B, W.data_ptr(), S, zsim.data_ptr(), err.data_ptr(),
                                 traj.data_ptr() if trajectory else 0, layout=self.layout, stream=st.cuda_stream)
        return zsim, err, traj

    def clearance(self, mesh, W=None, samples: int = 16, cull: Optional[bool] = None, positions: bool = True,
                  stream=None):
        '''
        Dense global positions of decision vectors and their signed distance to an obstacle mesh
        (ato_clearance, asynchronous on `stream`): per interval S1 = samples + 1 points of the collocation
        polynomial at i / samples (samples = 0: the K + 1 nodes, the reference's collision test), parametric
        problems placed through the centreline at the sample's own s. mesh: a MeshObstacle, or None for the
        positions alone. W as in replay(). cull: tile culling of the distance kernel (None: the measured
        default, obstacles.mesh_obstacle.DEFAULT_CULL); it does not change the result. Returns (pos, dist) in
        the layout: interleaved (3, N, S1, B), (N, S1, B); instance-major (B, N, S1, 3), (B, N, S1); dist is
        None without a mesh; positions=False keeps the positions in a buffer of the library and returns None
        for them. RK4-transcribed problems raise NotImplementedError.
        '''
        from aircraft_trajectory_optimization_amd.obstacles.mesh_obstacle import DEFAULT_CULL
        sp_, B = self.spec, self.batch
        il = self.layout == native.ATO_LAYOUT_INTERLEAVED
        W = self._columns(W, 'clearance')
        if mesh is None and not positions:
            raise ValueError('nothing to compute: no mesh and no positions')
        self._ensure_line()
        S = int(samples)
        S1 = self._sample_points(S)
        opts = {'device': self.device, 'dtype': torch.float64}
        pos = torch.empty((3, sp_.N, S1, B) if il else (B, sp_.N, S1, 3), **opts) if positions else None
        dist = torch.empty((sp_.N, S1, B) if il else (B, sp_.N, S1), **opts) if mesh is not None else None
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.problem.clearance_ptrs(B, W.data_ptr(), S, pos.data_ptr() if positions else 0,
                                    dist.data_ptr() if mesh is not None else 0,
                                    mesh.handle if mesh is not None else None,
                                    cull=int(DEFAULT_CULL if cull is None else bool(cull)), layout=self.layout,
                                    stream=st.cuda_stream)
        return pos, dist

    def audit(self, W=None, samples: int = 16, lb=None, ub=None, stream=None) -> torch.Tensor:
        '''
        Everything the NLP constrains at a node, evaluated at S1 points of every interval (ato_audit,
        asynchronous on `stream`): S1 = samples + 1 points of the collocation polynomial at i / samples
        (samples = 0: the K + 1 nodes), parametric problems with the geometry at the sample's own s. W as in
        replay(). lb, ub: bounds per component of the node vector (raceline.audit.path_bounds), (NV,) shared or
        (B, NV) per instance, host arrays or device tensors; None: no bounds (+inf in channels 0-5). Returns
        val in the layout: interleaved (NCH, N, S1, B), instance-major (B, N, S1, NCH); the channels are listed
        in include/ato.h. One stream per problem handle: the weight tables are handle state. RK4-transcribed
        problems raise NotImplementedError.
        '''
        sp_, B = self.spec, self.batch
        il = self.layout == native.ATO_LAYOUT_INTERLEAVED
        W = self._columns(W, 'audit')
        if (lb is None) != (ub is None):
            raise ValueError('lb and ub must both be given or both be None')
        per = False
        if lb is not None:
            lb, ub = ((v.to(torch.float64) if torch.is_tensor(v) else torch.as_tensor(np.array(v, np.float64)))
                      .to(self.device) for v in (lb, ub))
            if lb.shape != ub.shape or tuple(lb.shape) not in ((sp_.nv,), (B, sp_.nv)):
                raise ValueError(f'lb and ub must both be ({sp_.nv},) or ({B}, {sp_.nv})')
            per = lb.dim() == 2
            if per and il:
                lb, ub = lb.T, ub.T
            lb, ub = lb.contiguous(), ub.contiguous()
        self._ensure_line()
        S = int(samples)
        S1 = self._sample_points(S)
        nch = native.ATO_AUDIT_NCH
        val = torch.empty((nch, sp_.N, S1, B) if il else (B, sp_.N, S1, nch), device=self.device, dtype=torch.float64)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if stream is not None:      # temporaries made on the current stream, read on another
            for t in (W, lb, ub):
                if t is not None:
                    t.record_stream(st)
        self.problem.audit_ptrs(B, W.data_ptr(), S, val.data_ptr(), lb.data_ptr() if lb is not None else 0,
                                ub.data_ptr() if ub is not None else 0, per, layout=self.layout,
                                stream=st.cuda_stream)
        return val

    def set_gates(self, planes: Optional[dict]):
        ''' the gates gatecheck() checks: {'centre' (G, 3), 'R' (G, 3, 3), 'd_max' (G,), 'shape' (G,)} as
        raceline.gates.gate_planes returns them (at most 64, copied); None: the problem's own '''
        with torch.cuda.device(self.device):
            self.problem.gatecheck_set_gates(planes)
        self._n_planes = None if planes is None else len(np.asarray(planes['d_max']).reshape(-1))

    def gatecheck(self, W=None, samples: int = 16, axial_tol: float = 1e-6, stream=None) -> torch.Tensor:
        '''
        Passage of the continuous trajectory through every gate's opening (ato_gatecheck, asynchronous on
        `stream`): sign changes of the axial coordinate between the S + 1 points of every interval at
        i / samples (samples in [1, 64]), refined by bisection of the collocation polynomial, parametric
        problems placed through the centreline at the point's own s. W as in audit(). axial_tol (m): on open
        lines the first and the last point count as crossings within it. The gates are the problem's own unless
        set_gates() replaced them. Returns val in the layout: interleaved (NCH, G, B), instance-major (B, G, NCH);
        the channels (n_cross, margin, interval, x, t, p2, p3, off, flag) are listed in include/ato.h. One
        stream per problem handle: the weight table and the position buffer are handle state. RK4-transcribed
        problems raise NotImplementedError; a problem without gates raises RuntimeError.
        '''
        B = self.batch
        il = self.layout == native.ATO_LAYOUT_INTERLEAVED
        W = self._columns(W, 'gatecheck')
        self._ensure_line()
        G = len(self.spec.gates) if self._n_planes is None else self._n_planes
        nch = native.ATO_GATECHECK_NCH
        val = torch.empty((nch, G, B) if il else (B, G, nch), device=self.device, dtype=torch.float64)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if stream is not None:      # a temporary made on the current stream, read on another
            W.record_stream(st)
        self.problem.gatecheck_ptrs(B, W.data_ptr(), int(samples), val.data_ptr(), float(axial_tol),
                                    layout=self.layout, stream=st.cuda_stream)
        return val

    def remesh_from(self, src: 'BatchedNLP', W_src, cols=None, stream=None) -> torch.Tensor:
        '''
        Transfer decision vectors of the batch `src` (the same scenario on a coarser mesh: this N a multiple
        of src's, any degree) to this batch's discretisation (ato_remesh, asynchronous on `stream`):
        h' = h / r, every node variable by the Lagrange interpolant of its source interval. W_src: fp64
        device tensor in src's layout ((nw, B) interleaved, (B, nw) instance-major) or a host array
        (B, nw). cols: the source column of every column of this batch (int tensor or sequence of length
        self.batch), None for the identity. Returns W in this batch's layout. Both batches share one
        layout. Problems the transfer does not cover raise NotImplementedError.
        '''
        if src.layout != self.layout:
            raise ValueError('source and destination batches must share one layout')
        il = self.layout == native.ATO_LAYOUT_INTERLEAVED
        Bs, Bd = src.batch, self.batch
        if not torch.is_tensor(W_src):
            t = torch.as_tensor(np.array(W_src, np.float64).reshape(Bs, -1))
            W_src = (t.T.contiguous() if il else t.contiguous()).to(self.device)
        if W_src.dtype != torch.float64 or \
                tuple(W_src.shape) != ((src.problem.nw, Bs) if il else (Bs, src.problem.nw)):
            raise ValueError("W_src must be fp64 in the layout of the source batch")
        W_src = W_src.to(self.device).contiguous()
        if cols is not None:
            cols = torch.as_tensor(cols).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(cols.shape) != (Bd,):
                raise ValueError(f'cols must have one entry per destination column ({Bd})')
        W = torch.empty((self.problem.nw, Bd) if il else (Bd, self.problem.nw), device=self.device,
                        dtype=torch.float64)
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.problem.remesh_ptrs(src.problem, Bs, Bd, W_src.data_ptr(), W.data_ptr(),
                                 cols.data_ptr() if cols is not None else 0, layout=self.layout,
                                 stream=st.cuda_stream)
        return W

    def _host(self, t: torch.Tensor) -> np.ndarray:
        a = t.detach().to('cpu', torch.float64).numpy()
        return a.T.copy() if self.layout == native.ATO_LAYOUT_INTERLEAVED else a

    def results(self):
        ''' (g (B, ng), jac values (B, nnz), f (B,), grad_f (B, nw)) on the host '''
        torch.cuda.synchronize(self.device)
        return self._host(self.g), self._host(self.jac), self.f.detach().cpu().double().numpy(), \
            self._host(self.grad_f)
