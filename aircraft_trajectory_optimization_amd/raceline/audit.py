'''
Audit of solved racelines between their collocation nodes on the device.

Every row and every variable bound of the NLP holds at the collocation nodes only; between them the degree-K
polynomial is unconstrained, and the last stretch (tau_K, 1] of every interval is an extrapolation. The replay
(raceline/replay.py) says whether a solution flies and the clearance (raceline/clearance.py) whether it hits
the mesh; this holds the polynomial itself against what the NLP asks of a node, at S + 1 points of every
interval (libato's ato_audit): the variable bounds (the corridor y, n among them), s' >= 0, the regularity of
the parametric frame, the point mass's thrust ball, and the ODE defect |f(z, u) - z'| of the problem's own
model variant (the relative attitude included, which the replay does not cover), parametric geometry taken at
the sample's own s rather than frozen at the node's nominal s as the NLP does.

What it does not look at: the obstacle-tube sphere rows (a per-node table; the clearance answers that on the
mesh), gates (raceline/gates.py asks the continuous trajectory about them) and closure rows (point constraints),
CPC progress variables, the dU rows (exact between the
nodes when they hold at them) and RK4 transcriptions. It says nothing about the arc between two samples: there
is no Lipschitz argument here as there is for distances. No solver path calls it.
'''
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from aircraft_trajectory_optimization_amd import native
from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec

MARGINS = ('pos', 'att', 'vel', 'rate', 'u', 'du', 'sdot', 'reg', 'stage')
DEFECTS = ('d_pos', 'd_att', 'd_vel', 'd_rate')
CHANNELS = MARGINS + DEFECTS + ('att_dev',)


@dataclass
class AuditResult:
    ''' device tensors of one audit of B instances; S1 points per interval '''
    val: torch.Tensor            # (NCH, N, S1, B) every channel at every sample
    margin: torch.Tensor         # (B, 9) minimum over (n, i) of channels 0-8; >= 0 means satisfied
    where: torch.Tensor          # (B, 9, 2) interval and sample of that minimum
    defect: torch.Tensor         # (B, 4) maximum over (n, i) of channels 9-12 (NaN where one is)
    att_dev: torch.Tensor        # (B,) maximum of channel 13
    passed: torch.Tensor         # (B,) bool: every margin >= -tol (a NaN margin fails). With force_regularity (the
                                 # configuration's default) channel 7 ('reg') is held at EVERY sample, while the NLP
                                 # has that row only at nodes of large nominal curvature: look at margin[:, 7]
                                 # separately before reading a failure as a violated constraint of the solve
    samples: int = 16
    tol: float = 0.0
    varying: str = 'raise'       # path_bounds' rule the bounds came from: 'raise' (every node's bound is the one
                                 # held) or 'outer' (the loosest over the nodes: `passed` is then a necessary check)


def path_bounds(spec: ProblemSpec, LBW=None, UBW=None, varying: str = 'raise'):
    '''
    Bounds per component of the node vector (z, u, du), as ato_audit holds every sample against them: (NV,)
    from bounds (nw,) (default: the problem's own lbw / ubw), (B, NV) from per-instance bounds (B, nw) such as
    corridor_bounds. The NLP bounds every node separately; a sample between nodes can only be held to a bound
    that is the same at all of them, so a component whose bound differs between nodes of one instance raises
    ValueError. varying='outer' takes the loosest bound over the nodes instead (a sample outside it violates
    every node's bound; one inside it proves nothing about the tighter nodes).
    '''
    if varying not in ('raise', 'outer'):
        raise ValueError("varying must be 'raise' or 'outer'")
    lbw = np.asarray(spec.lbw if LBW is None else LBW, float)
    ubw = np.asarray(spec.ubw if UBW is None else UBW, float)
    if lbw.shape != ubw.shape or lbw.shape[-1] != spec.nw or lbw.ndim > 2:
        raise ValueError(f'bounds must be ({spec.nw},) or (B, {spec.nw})')
    a, b = spec.N, spec.N + spec.P * spec.nv
    lo = lbw[..., a:b].reshape(lbw.shape[:-1] + (spec.P, spec.nv))
    hi = ubw[..., a:b].reshape(lo.shape)
    if varying == 'raise':
        bad = np.any(lo != lo[..., :1, :], axis=-2) | np.any(hi != hi[..., :1, :], axis=-2)
        if np.any(bad):
            comps = sorted(set(np.nonzero(bad)[-1].tolist()))
            raise ValueError(f'the bounds of node-vector components {comps} differ between nodes: samples between '
                             "nodes have no bound to be held to (varying='outer' takes the loosest)")
    return np.ascontiguousarray(lo.min(axis=-2)), np.ascontiguousarray(hi.max(axis=-2))


def reduce_audit(val: torch.Tensor, samples: int, tol: float = 0.0, varying: str = 'raise') -> AuditResult:
    ''' the per-instance reductions of val (NCH, N, S1, B): torch ops on its device '''
    nch, N, S1, B = val.shape
    nm = len(MARGINS)
    flat = val.reshape(nch, N * S1, B)
    m = flat[:nm]
    nan = torch.isnan(m)
    # torch.min propagates NaN but leaves its index open: find the first NaN (else the minimum) by hand
    key = torch.where(nan, torch.full_like(m, -float('inf')), m)
    idx = key.argmin(dim=1)                                             # (9, B)
    margin = torch.gather(m, 1, idx[:, None, :])[:, 0, :]
    where = torch.stack([idx // S1, idx % S1], dim=-1).permute(1, 0, 2).contiguous()
    defect = flat[nm:nm + len(DEFECTS)].amax(dim=1)                     # amax propagates NaN
    att_dev = flat[nm + len(DEFECTS)].amax(dim=0)
    passed = (margin >= -float(tol)).all(dim=0)
    return AuditResult(val=val, margin=margin.T.contiguous(), where=where, defect=defect.T.contiguous(),
                       att_dev=att_dev, passed=passed, samples=int(samples), tol=float(tol), varying=varying)


def audit_solutions(spec: ProblemSpec, X, samples: int = 16, LBW=None, UBW=None, tol: float = 0.0,
                    device: Optional[torch.device] = None, varying: str = 'raise') -> AuditResult:
    '''
    Audit decision vectors X of the problem `spec`: a host array (B, nw) (or one vector (nw,)), or a device
    tensor (nw, B) as the batched solver returns its x.

    samples = S >= 1: S + 1 points per interval of the collocation polynomial at i / S, both ends; samples = 0:
    the K + 1 nodes, where the margins are the NLP's own (up to the geometry, which is taken at the node's own
    s). LBW / UBW: the bounds the solve ran under, (nw,) or per instance (B, nw) (default: the problem's own),
    reduced by path_bounds(varying=...). passed = every margin >= -tol; the defects are reported, not judged
    (at a collocation node they are the NLP's residual plus the frozen-geometry error, between nodes the
    polynomial's distance from the ODE).
    '''
    if torch.is_tensor(X):
        X = X.reshape(X.shape[0], -1).to(torch.float64)
        B = X.shape[1]
    else:
        X = np.atleast_2d(np.asarray(X, np.float64))
        B = X.shape[0]
    lb, ub = path_bounds(spec, LBW, UBW, varying=varying)
    nlp = BatchedNLP(spec, B, layout=native.ATO_LAYOUT_INTERLEAVED, device=device, buffers=False)
    if torch.is_tensor(X):
        X = X.to(nlp.device)
    with torch.cuda.device(nlp.device):
        val = nlp.audit(X, samples=int(samples), lb=lb, ub=ub)
        return reduce_audit(val, int(samples), tol, varying)
