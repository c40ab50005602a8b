'''
ORACLE (test infrastructure only) of the Lagrange basis over the collocation nodes tau_0 .. tau_K, in numpy: the
one restatement the replay, mesh-transfer, clearance and audit oracles share. Independent of csrc/ato_sample.hpp
(it calls no twin): only the formulas stated in include/ato.h are shared, product by product in the same order, so
the twins' tables can be asserted equal to these.
'''
import numpy as np


def basis(tau, x):
    ''' l_j(x), j = 0 .. K: the product over r != j (ascending) of (x - tau_r) / (tau_j - tau_r) '''
    out = np.ones(len(tau))
    for j in range(len(tau)):
        for r in range(len(tau)):
            if r != j:
                out[j] *= (x - tau[r]) / (tau[j] - tau[r])
    return out


def dbasis(tau, x):
    ''' l_j'(x) = sum over m != j of 1 / (tau_j - tau_m) prod over r != j, m of (x - tau_r) / (tau_j - tau_r), m and
    r ascending '''
    out = np.zeros(len(tau))
    for j in range(len(tau)):
        for m in range(len(tau)):
            if m == j:
                continue
            v = 1.0 / (tau[j] - tau[m])
            for r in range(len(tau)):
                if r not in (j, m):
                    v *= (x - tau[r]) / (tau[j] - tau[r])
            out[j] += v
    return out


def table(tau, xs, fn=basis):
    ''' [len(xs)][K + 1]: fn(tau, x) for every abscissa x '''
    tau = np.asarray(tau, float)
    return np.array([fn(tau, float(x)) for x in xs]).reshape(len(xs), len(tau))
