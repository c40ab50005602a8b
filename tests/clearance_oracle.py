'''
ORACLE (test infrastructure only) of the clearance: numpy restatement of the sample abscissae, the Lagrange
basis (tests/lagrange_oracle.py) and the Lagrange sum, the product's own line.p2x for the lift (one call over all samples) and
oracle.ref_mesh.signed_distance for the distance (another closest-point algorithm and another ray
direction than the kernels).
'''
import numpy as np

from oracle import ref_mesh
from tests import lagrange_oracle


def abscissae(spec, samples):
    return np.asarray(spec.tau, float) if samples == 0 else np.arange(samples + 1) / samples


def weights(spec, samples):
    ''' [S1][K1] l_j(x_i) '''
    return lagrange_oracle.table(spec.tau, abscissae(spec, samples))


def positions(spec, W, samples):
    ''' W (B, nw) -> (B, N, S1, 3) global positions '''
    W = np.atleast_2d(np.asarray(W, float))
    B = W.shape[0]
    wt = weights(spec, samples)
    Z = W[:, spec.N:spec.N + spec.P * spec.nv].reshape(B, spec.N, spec.K1, spec.nv)[..., :3]
    q = np.einsum('ij,bnjc->bnic', wt, Z)
    if not spec.param:
        return q
    flat = q.reshape(-1, 3)
    return spec.line.p2x(flat[:, 0], flat[:, 1], flat[:, 2]).T.reshape(q.shape)


def node_positions(spec, W):
    ''' p2x of the node states themselves: what _unpack feeds the reference's collision test '''
    W = np.atleast_2d(np.asarray(W, float))
    Z = W[:, spec.N:spec.N + spec.P * spec.nv].reshape(W.shape[0], spec.N, spec.K1, spec.nv)[..., :3]
    if not spec.param:
        return Z
    flat = Z.reshape(-1, 3)
    return spec.line.p2x(flat[:, 0], flat[:, 1], flat[:, 2]).T.reshape(Z.shape)


def signed_distance(X, V, F):
    return ref_mesh.signed_distance(np.asarray(X, float).reshape(-1, 3), np.asarray(V, float), np.asarray(F))


def box_mesh(lo, hi):
    ''' (V (8, 3), F (12, 3)) of an axis-aligned box, outward orientation '''
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    V = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
    F = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4],
                  [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]], np.int32)
    return V, F


def lattice_mesh(n_boxes=64, pitch=(1.0, 1.0, 1.0), side=(0.4, 0.4, 0.4), origin=(0.0, 0.0, 0.0)):
    ''' the first n_boxes boxes of a 4 x 4 x 4 lattice: 12 n_boxes triangles '''
    pitch, side, origin = (np.asarray(v, float) for v in (pitch, side, origin))
    Vs, Fs = [], []
    for m in range(n_boxes):
        c = origin + pitch * np.array([m % 4, (m // 4) % 4, m // 16], float)
        V, F = box_mesh(c - side / 2, c + side / 2)
        Fs.append(F + 8 * m)
        Vs.append(V)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)
