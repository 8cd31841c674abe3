"""The matcher beyond 256 queries, without a GPU: the host solver -- the reference the device solver is held to in
tests/test_many_queries_gpu.py -- against scipy at the extents the device entry point now takes (up to 1024 x 1024),
and the entry point's refusal of anything larger before it touches a device."""
import numpy as np
import pytest
import torch


def tie_costs(M, ld, Lv, seed):
    """f32 [Lv, B=2, M, ld] with the tie constructions of test_device_lap_is_bit_identical_to_the_host_solver_and_scipy:
    level 0 a duplicated column, level 1 (if any) rounded small-integer costs, level 2 (if any) duplicated rows."""
    rng = np.random.default_rng(seed)
    cost = torch.from_numpy(rng.standard_normal((Lv, 2, M, ld)).astype(np.float32) * 3)
    if ld > 1:
        cost[0, :, :, 1] = cost[0, :, :, 0]
    if Lv > 1:
        cost[1] = torch.round(cost[1])
    if Lv > 2:
        cost[2, :, 1::2] = cost[2, :, 0::2][:, : cost[2, :, 1::2].shape[1]]
    return cost


def assert_equals_scipy(match, cost, n):
    """match i32 [M] (local column or -1) is scipy's assignment of cost[:, :n]."""
    from scipy.optimize import linear_sum_assignment
    i, j = linear_sum_assignment(cost[:, :n].numpy())
    assert np.array_equal(np.nonzero(match.numpy() >= 0)[0], i)
    assert np.array_equal(match[match >= 0].numpy(), j)


@pytest.mark.parametrize("M,n", [(300, 37), (300, 256), (300, 300), (1024, 17), (1024, 1024)])
def test_host_solver_equals_scipy_at_the_new_extents(M, n):
    from future_od.native import ops
    Lv = 3
    cost = tie_costs(M, n, Lv, seed=M * 7919 + n)[:, 0].contiguous()          # [Lv, M, n]: one sample per level
    got = ops.lap_solve_batch_host(cost, [n] * Lv, threads=3)
    for lv in range(Lv):
        assert_equals_scipy(got[lv], cost[lv], n)


def test_device_solver_refuses_extents_beyond_the_limit_before_any_launch():
    from future_od.native import lib as L
    assert L.LAP_MAX_DIM == 1024 and type(L.LAP_STAGE_FLOATS) is int and L.LAP_STAGE_FLOATS >= 300 * 40
    cost = torch.zeros(4)                                          # host memory: never read, the refusal comes first
    off, match, status = (torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                          torch.zeros(1, dtype=torch.int32))
    args = lambda M, ld: (cost.data_ptr(), 1, 1, M, ld, off.data_ptr(), match.data_ptr(), status.data_ptr(), None)
    for M, ld in ((1025, 8), (8, 1025), (1025, 1025), (4096, 300)):
        rc = L.LIB.fod_lap_solve_batch_dev(*args(M, ld))
        assert rc == L.ERR_ARG, (M, ld, rc)
        msg = L.last_error()
        assert f"M={M}" in msg and f"ld_n={ld}" in msg and "1024" in msg, msg
    rc = L.LIB.fod_lap_solve_batch_dev(None, 1, 1, 300, 256, off.data_ptr(), match.data_ptr(), status.data_ptr(), None)
    assert rc == L.ERR_ARG and "null" in L.last_error()
    assert int(status[0]) == 0 and not match.any()
