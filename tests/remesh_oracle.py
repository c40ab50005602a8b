'''
Test-side oracle of the mesh transfer (numpy): the Lagrange basis of tests/lagrange_oracle.py and the triple loop
of the definition in include/ato.h. Independent of csrc/ato_remesh.hpp: only the definition is shared.
'''
import numpy as np

from tests.lagrange_oracle import basis


def weights(tau_s, tau_d, r):
    ''' [r][K' + 1][K + 1]: l_m((j + tau'_k) / r) '''
    return np.array([[basis(tau_s, (float(j) + tau_d[k]) / float(r)) for k in range(len(tau_d))] for j in range(r)])


def remesh(src, dst, W):
    ''' decision vectors W (B, nw) of the spec src -> (B, nw') of the spec dst '''
    W = np.atleast_2d(np.asarray(W, float))
    B, N, r, nv = W.shape[0], src.N, dst.N // src.N, src.nv
    V = W[:, N:N + N * src.K1 * nv].reshape(B, N, src.K1, nv)
    wt = weights(src.tau, dst.tau, r)
    out = np.zeros((B, N, r, dst.K1, nv))
    for j in range(r):
        for k in range(dst.K1):
            for m in range(src.K1):
                out[:, :, j, k] += wt[j, k, m] * V[:, :, m]
    h = np.repeat(W[:, :N] / float(r), r, axis=1)
    return np.concatenate([h, out.reshape(B, -1)], axis=1)


def dense(spec, w, n, x):
    ''' the interpolant of interval n at interval time x in [0, 1]: (nv,) '''
    V = np.asarray(w, float)[spec.N:spec.N + spec.N * spec.K1 * spec.nv].reshape(spec.N, spec.K1, spec.nv)
    return basis(spec.tau, x) @ V[n]
