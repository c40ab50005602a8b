'''
Test-side oracle of the replay (numpy): classical RK4 over oracle.ref_models with frame='global',
the Lagrange basis of tests/lagrange_oracle.py, lifting through the Python centreline. Independent of
csrc/ato_replay.hpp: only the definition in include/ato.h is shared.
'''
import numpy as np

from oracle import ref_models
from tests import lagrange_oracle


def weights(tau, S):
    ''' l_j(i / (2 S)), i = 0 .. 2 S '''
    return lagrange_oracle.table(tau, [float(i) / float(2 * S) for i in range(2 * S + 1)])


def _veh(spec):
    v = spec.vehicle
    d = {'m': v.m, 'g': v.g, 'b1': v.b1, 'b2': v.b2, 'b3': v.b3}
    if spec.is_drone:
        d.update({'I1': v.I1, 'I2': v.I2, 'I3': v.I3, 'bw1': v.bw1, 'bw2': v.bw2, 'bw3': v.bw3, 'l': v.l, 'k': v.k})
    return d


def _att(spec):
    return 'dcm' if spec.use_dcm else bool(spec.vehicle.use_quat)


def zdot(spec, z, u):
    ''' global-model ODE, z (nz, M), u (nu, M) '''
    if spec.is_drone:
        return ref_models.drone_zdot(z, u, _veh(spec), _att(spec), 'global', True)
    return ref_models.point_zdot(z, u, _veh(spec), 'global', True)


def lift(spec, Z, s):
    ''' problem-frame states Z (M, nz) at path lengths s (M,) -> global-model states '''
    Z = np.array(Z, float)
    if not spec.param:
        return Z
    s = np.asarray(s, float)
    xc, ey, en = spec.line.p2xc(s), spec.line.p2ey(s), spec.line.p2en(s)     # (3, M)
    Z[:, :3] = (xc + Z[:, 1] * ey + Z[:, 2] * en).T
    return Z


def rotation(spec, r):
    ''' r (nr, M) -> R (3, 3, M) '''
    att = _att(spec)
    return ref_models.dcm_R(r) if att == 'dcm' else ref_models.esp_R(r) if att else ref_models.ypr_R(r)


def errors(spec, zsim, zref):
    ''' (M, nz) simulated / reference global states -> (M, 4): |dp|, attitude angle, |dv|, |dw| '''
    out = np.zeros((zsim.shape[0], 4))
    out[:, 0] = np.linalg.norm(zsim[:, :3] - zref[:, :3], axis=1)
    if spec.is_drone:
        nr = spec.nz - 9
        Ra, Rb = rotation(spec, zsim[:, 3:3 + nr].T), rotation(spec, zref[:, 3:3 + nr].T)
        E = np.einsum('kim,kjm->ijm', Ra, Rb)
        vee = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
        out[:, 1] = np.arctan2(0.5 * np.linalg.norm(vee, axis=0), 0.5 * (E[0, 0] + E[1, 1] + E[2, 2] - 1.0))
        out[:, 2] = np.linalg.norm(zsim[:, 3 + nr:6 + nr] - zref[:, 3 + nr:6 + nr], axis=1)
        out[:, 3] = np.linalg.norm(zsim[:, 6 + nr:9 + nr] - zref[:, 6 + nr:9 + nr], axis=1)
    else:
        out[:, 2] = np.linalg.norm(zsim[:, 3:6] - zref[:, 3:6], axis=1)
    return out


def replay(spec, w, S):
    ''' one decision vector -> zsim (N, nz), err (N, 4), traj (N, S, nz) '''
    w = np.asarray(w, float)
    N, K1, nz, nu = spec.N, spec.K1, spec.nz, spec.nu
    h = w[:N]
    nodes = w[N:N + N * K1 * spec.nv].reshape(N, K1, spec.nv)       # CPC variables after it are ignored
    Z, U = nodes[:, :, :nz], nodes[:, :, nz:nz + nu]
    lw = weights(spec.tau, S)
    s = np.asarray(spec.interval_s, float)
    z = lift(spec, Z[:, 0], s[:N]).T                                 # (nz, N): the intervals are the batch axis
    hs = h / S
    traj = np.zeros((N, S, nz))
    for i in range(S):
        ua, um, ub = (np.einsum('j,njm->mn', lw[2 * i + q], U) for q in range(3))
        k1 = zdot(spec, z, ua)
        k2 = zdot(spec, z + 0.5 * hs * k1, um)
        k3 = zdot(spec, z + 0.5 * hs * k2, um)
        k4 = zdot(spec, z + hs * k3, ub)
        z = z + hs / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        traj[:, i] = z.T
    zsim = z.T
    zref = lift(spec, np.einsum('k,nki->ni', spec.D, Z), s[1:N + 1])
    return zsim, errors(spec, zsim, zref), traj
