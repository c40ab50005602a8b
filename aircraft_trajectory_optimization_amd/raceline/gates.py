'''
Gate passage of solved racelines on the device.

A gate row of the NLP is a point constraint: it holds at one abscissa of one interval -- node Z[interval, 0] in the
global frame; in the parametric frame the Lagrange point d of the interval that contains the gate's nominal s,
where y and n are placed through a frame frozen at the gate's s while the trajectory's own s at that abscissa is
free. The replay (raceline/replay.py) says whether a solution flies, the clearance (raceline/clearance.py) whether
it hits the mesh, the audit (raceline/audit.py) whether the polynomial keeps its bounds between the nodes; this
asks the continuous trajectory what a racing user asks first: does it go through each gate's opening, where, and
when (libato's ato_gatecheck). Per gate it finds every crossing of the gate's plane between S + 1 points of every
interval, refines it by bisection of the collocation polynomial (lifted through the centreline at the point's own
s in parametric problems), and reports the crossing with the largest margin d_max - |lateral offset|.

What it does not look at: the trajectory as flown (the replay), RK4 transcriptions, closure rows, the gate's
frame as an obstacle, and the order of the gates (the passage time t is reported, not judged). The direction of a
crossing is recorded, not required: gate_orientation snaps e1 to "up" and a track may dive through a gate. Two
crossings inside one sample step cancel and are not seen. No solver path calls it.
'''
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from aircraft_trajectory_optimization_amd import native
from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec

CHANNELS = ('n_cross', 'margin', 'interval', 'x', 't', 'p2', 'p3', 'off', 'flag')


@dataclass
class GatePassageResult:
    ''' device tensors of one gate check of B instances at G gates '''
    val: torch.Tensor            # (NCH, G, B) every channel, as ato_gatecheck wrote it
    n_cross: torch.Tensor        # (B, G) crossings of the gate's plane found
    margin: torch.Tensor         # (B, G) margin of the best crossing (>= 0: inside the opening); -inf: none
    interval: torch.Tensor       # (B, G) interval of the best crossing (-1: none)
    x: torch.Tensor              # (B, G) its abscissa in [0, 1]
    t: torch.Tensor              # (B, G) passage time: sum of h before the interval + x h
    p2: torch.Tensor             # (B, G) lateral offsets along the gate's e2, e3
    p3: torch.Tensor
    off: torch.Tensor            # (B, G) sqrt(p2^2 + p3^2) (the exact row of a fix_center gate)
    flag: torch.Tensor           # (B, G) +1 / -1 direction along e1; 0: no crossing; NaN: a non-finite value was met
    missed: torch.Tensor         # (B, G) bool: no crossing, a NaN flag, or margin < -tol
    passed: torch.Tensor         # (B,) bool: no gate missed
    samples: int = 16
    tol: float = 0.0


def gate_planes(spec: ProblemSpec) -> dict:
    ''' the problem's own gates as ato_gatecheck reads them: {'centre' (G, 3), 'R' (G, 3, 3) with columns e1 e2 e3,
    'd_max' (G,), 'shape' (G,) int32 (native.ATO_GATE_*)}, in the order of spec.gates '''
    G = len(spec.gates)
    return {'centre': np.array([g['gate_x'] for g in spec.gates], float).reshape(G, 3),
            'R': np.array([np.asarray(g['R'], float).reshape(3, 3) for g in spec.gates], float).reshape(G, 3, 3),
            'd_max': np.array([g['d_max'] for g in spec.gates], float).reshape(G),
            'shape': np.array([g['shape'] for g in spec.gates], np.int32).reshape(G)}


def gate_points(spec: ProblemSpec):
    ''' where the NLP itself holds every gate: (interval (G,) int, abscissa (G,) in [0, 1]). The gate's weights are
    l_k(d) on the interval's nodes, and a Lagrange basis reproduces the abscissa: d = sum_k l_k(d) tau_k (0 for
    the global frame's node Z[interval, 0], 1 for a gate on the end of the horizon) '''
    tau = np.asarray(spec.tau, float)
    n = np.array([g['interval'] for g in spec.gates], np.int64)
    d = np.array([float(np.asarray(g['coef'], float)[:g['n_coef']] @ tau[:g['n_coef']]) for g in spec.gates], float)
    return n, d


def reduce_gates(val: torch.Tensor, samples: int, tol: float = 0.0) -> GatePassageResult:
    ''' the named channels and the verdicts of val (NCH, G, B): torch ops on its device '''
    ch = {name: val[i].T.contiguous() for i, name in enumerate(CHANNELS)}
    missed = ~((ch['n_cross'] >= 1) & torch.isfinite(ch['flag']) & (ch['margin'] >= -float(tol)))
    return GatePassageResult(val=val, missed=missed, passed=~missed.any(dim=1), samples=int(samples),
                             tol=float(tol), **ch)


def gate_passage(spec: ProblemSpec, X, samples: int = 16, tol: float = 0.0, gates: Optional[dict] = None,
                 device: Optional[torch.device] = None, axial_tol: float = 1e-6) -> GatePassageResult:
    '''
    Gate passage of decision vectors X of the problem `spec`: a host array (B, nw) (or one vector (nw,)), or a
    device tensor (nw, B) as the batched solver returns its x.

    samples = S in [1, 64]: the crossings are looked for between S + 1 points per interval at i / S and refined by
    bisection. gates: planes in the form of gate_planes() to check instead of the problem's own (a tighter
    d_max, CPC waypoints as circular gates); at most 64. passed = every gate has a crossing, a finite flag and
    margin >= -tol. axial_tol (m): on open lines the first and the last point count as crossings within it.
    '''
    if torch.is_tensor(X):
        X = X.reshape(X.shape[0], -1).to(torch.float64)
        B = X.shape[1]
    else:
        X = np.atleast_2d(np.asarray(X, np.float64))
        B = X.shape[0]
    nlp = BatchedNLP(spec, B, layout=native.ATO_LAYOUT_INTERLEAVED, device=device, buffers=False)
    if gates is not None:
        nlp.set_gates(gates)
    if torch.is_tensor(X):
        X = X.to(nlp.device)
    with torch.cuda.device(nlp.device):
        val = nlp.gatecheck(X, samples=int(samples), axial_tol=axial_tol)
        return reduce_gates(val, int(samples), tol)
