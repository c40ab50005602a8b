'''
Pins of the sampling layer's weight tables (csrc/ato_sample.hpp), on the CPU: the tables the four twins hand out
against tests/golden/sample_layer/tables.npz, recorded from the twins before the replay, mesh-transfer, clearance
and audit tables were folded into one Lagrange row function. The arithmetic is IEEE multiplication and division in
a fixed order and the twins are compiled without contraction, so the tables are asserted equal, bit for bit.
'''
import os

import numpy as np
import pytest

from tests.audit_helpers import AuditTwin
from tests.clearance_helpers import ClearanceTwin, case_spec as clearance_spec
from tests.helpers import REPO
from tests.remesh_helpers import RemeshTwin, mesh_spec
from tests.replay_helpers import ReplayTwin, case_spec as replay_spec

GOLDEN = os.path.join(REPO, 'tests', 'golden', 'sample_layer', 'tables.npz')
DEGREES = (1, 2, 9)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN))


def same(a, b):
    ''' equal shapes and equal bits '''
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('K', DEGREES)
def test_replay_tables_are_pinned(golden, K):
    tw = ReplayTwin(replay_spec('point', 'parametric', K))
    for S in (1, 16, 64):
        assert same(tw.weights(S), golden[f'replay_K{K}_S{S}']), S


@pytest.mark.parametrize('K', DEGREES)
def test_clearance_and_audit_tables_are_pinned(golden, K):
    spec = clearance_spec('race', 'point', 'parametric', K)
    ct, at = ClearanceTwin(spec), AuditTwin(spec)
    for S in (0, 1, 5, 64):
        wt, dw = at.weights(S)
        assert same(ct.weights(S), golden[f'clearance_K{K}_S{S}']), S
        assert same(wt, golden[f'audit_wt_K{K}_S{S}']) and same(dw, golden[f'audit_dw_K{K}_S{S}']), S
        assert same(wt, ct.weights(S)), S
    # at the nodes: exact deltas, and the problem's own derivative table, dw[k][j] = C[j][k]
    wt, dw = at.weights(0)
    assert np.array_equal(wt, np.eye(K + 1))
    assert np.array_equal(dw, np.array(spec.C, float).reshape(K + 1, K + 1).T)


@pytest.mark.parametrize('K', DEGREES)
def test_remesh_tables_are_pinned(golden, K):
    src = mesh_spec('point', 'parametric', 3, K)
    for r in (1, 2, 3):
        for Kd in (1, 9):
            wt = RemeshTwin(src, mesh_spec('point', 'parametric', 3 * r, Kd)).weights()
            assert same(wt, golden[f'remesh_K{K}_r{r}_Kd{Kd}']), (r, Kd)
