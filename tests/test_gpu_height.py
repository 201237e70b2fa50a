"""rti_height_from_normals on the GPU against the NumPy restatement (tests/height_ref.py): the mask, the NaN pattern,
the gauge, the solution within the bound of a residual of the requested size, for both preconditioners and both
normal layouts at the smallest shapes at which each mechanism can go wrong; then determinism, flip_y, the start
vector, the iteration limits and the torch op."""
import functools

import numpy as np
import pytest
import torch

import height_ref as hr
import rti

pytestmark = pytest.mark.gpu

RTOL, MAX_ITERS = 1e-10, 5000
EMPTY = ("1x1", "nan5x5")


def as_layout(n, layout, dev):
    t = torch.as_tensor(n, device=dev)
    return t.permute(2, 0, 1).contiguous() if layout == "planar" else t


@functools.lru_cache(maxsize=None)
def solved(name, precond, layout, check_every=1):
    """(height, valid, stats) of one call, as NumPy arrays; cached so that the checks share the solves."""
    dev = torch.device("cuda", 0)
    st = np.full(6, -7.0)
    z, v = rti.height_from_normals(as_layout(hr.case(name).n, layout, dev), rtol=RTOL, max_iters=MAX_ITERS,
                                   precond=precond, layout=layout, return_valid=True, stats=st,
                                   check_every=check_every)
    assert z.dtype == torch.float32 and v.dtype == torch.uint8 and z.shape == v.shape == hr.case(name).n.shape[:2]
    return z.cpu().numpy(), v.cpu().numpy(), st


def check_solution(pr, z, st, rtol=RTOL):
    """The bound of the issue: a residual of rtol·‖b‖ moves the solution by at most rtol·‖b‖₂/λ₂ in the 2-norm,
    hence per pixel, and the fp32 output adds 2⁻²³·max|z_ref|; each component's mean difference is removed."""
    bound = rtol * pr.norm_b / pr.lambda2 + 2.0 ** -23 * np.nanmax(np.abs(pr.z))
    err = np.abs(pr.align(z) - pr.z)[pr.valid].max()
    print(f"err {err:.3e} bound {bound:.3e} iters {st[0]:.0f} met {st[1]:.0f} rec {st[2]:.2e} true {st[3]:.2e}")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("layout", ["pixel", "planar"])
@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
@pytest.mark.parametrize("name", hr.CASES)
def test_height_matches_reference(cuda, name, precond, layout):
    pr = hr.case(name)
    z, v, st = solved(name, precond, layout)
    assert np.array_equal(v.astype(bool), pr.valid) and set(np.unique(v)) <= {0, 1}
    assert np.array_equal(np.isnan(z), ~pr.valid) and np.isfinite(z[pr.valid]).all()
    assert st[4] == pr.valid.sum()
    if name in EMPTY:
        assert st[0] == 0 and not pr.valid.any()
        return
    assert abs(st[5] - pr.norm_b) <= 1e-14 * pr.norm_b
    assert st[1] >= 0 and st[0] >= st[1] and st[0] <= MAX_ITERS
    zv = z[pr.valid].astype(np.float64)
    assert abs(zv.mean()) <= 2.0 ** -22 * np.abs(zv).max()
    check_solution(pr, z, st)
    assert st[3] <= 10 * RTOL and st[2] <= RTOL * (1 + 1e-12)


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
@pytest.mark.parametrize("name", hr.CASES)
def test_layouts_and_runs_give_identical_bits(cuda, name, precond):
    a, b = solved(name, precond, "pixel"), solved(name, precond, "planar")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[2], b[2])
    if name in ("37x41", "33x130"):  # a second run of the same call, not the cached one
        n = torch.as_tensor(hr.case(name).n, device=cuda)
        st = np.zeros(6)
        z = rti.height_from_normals(n, rtol=RTOL, max_iters=MAX_ITERS, precond=precond, stats=st, check_every=1)
        assert np.array_equal(z.cpu().numpy().view(np.uint32), a[0].view(np.uint32)) and np.array_equal(st, a[2])


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
def test_flip_y_is_the_negated_map(cuda, precond):
    n = hr.case("37x41").n
    neg = n.copy()
    neg[..., 1] = -neg[..., 1]
    kw = dict(rtol=RTOL, max_iters=MAX_ITERS, precond=precond)
    a = rti.height_from_normals(torch.as_tensor(n, device=cuda), flip_y=True, **kw).cpu().numpy()
    b = rti.height_from_normals(torch.as_tensor(neg, device=cuda), **kw).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a.view(np.uint32), solved("37x41", precond, "pixel")[0].view(np.uint32))
    pr = hr.Problem(n, flip_y=True)
    check_solution(pr, a, np.zeros(6))


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
def test_flat_map_is_exactly_zero(cuda, precond):
    n = torch.zeros((19, 23, 3), device=cuda)
    n[..., 2] = 1.0
    st = np.full(6, -7.0)
    z, v = rti.height_from_normals(n, precond=precond, return_valid=True, stats=st,
                                   z0=torch.full((19, 23), 3.5, device=cuda))
    assert not z.cpu().numpy().view(np.uint32).any() and v.cpu().numpy().all()
    assert list(st) == [0, 0, 0, 0, 19 * 23, 0]


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
def test_start_from_a_converged_solution(cuda, precond):
    """z0 = the fp32 output of a converged solve.  Its own residual is the fp32 rounding pushed through A: at most
    8·2⁻²⁴·max|z| per pixel (degree 4, four neighbours), ‖r‖ <= 2⁻²¹·max|z|·sqrt(valid), which the test holds
    against rtol·‖b‖ for rtol = 1e-3 before it relies on it; the call then returns within check_every iterations."""
    pr = hr.case("37x41")
    z, _, _ = solved("37x41", precond, "pixel")
    rtol, every = 1e-3, 4
    assert 2.0 ** -21 * np.nanmax(np.abs(z)) * np.sqrt(pr.valid.sum()) <= rtol * pr.norm_b
    st = np.zeros(6)
    z0 = torch.as_tensor(np.nan_to_num(z), device=cuda)
    out = rti.height_from_normals(torch.as_tensor(pr.n, device=cuda), rtol=rtol, max_iters=100, precond=precond, z0=z0,
                                  stats=st, check_every=every)
    assert st[0] <= every and st[1] == 0 and st[2] <= rtol
    assert np.nanmax(np.abs(out.cpu().numpy() - z)) <= 2.0 ** -22 * np.nanmax(np.abs(z))
    # a start with NaN at invalid pixels is read only at the valid ones
    st2 = np.zeros(6)
    out2 = rti.height_from_normals(torch.as_tensor(pr.n, device=cuda), rtol=rtol, max_iters=100, precond=precond,
                                   z0=torch.as_tensor(z, device=cuda), stats=st2, check_every=every)
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), out.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
def test_iteration_limits(cuda, precond):
    pr = hr.case("37x41")
    n = torch.as_tensor(pr.n, device=cuda)
    st = np.zeros(6)
    z = rti.height_from_normals(n, rtol=1e-14, max_iters=3, precond=precond, stats=st, check_every=8)
    assert st[0] == 3 and st[1] == -1 and st[2] > 1e-14 and np.array_equal(np.isnan(z.cpu().numpy()), ~pr.valid)
    st0 = np.zeros(6)
    z = rti.height_from_normals(n, rtol=RTOL, max_iters=0, precond=precond, stats=st0)
    assert st0[0] == 0 and st0[1] == -1 and abs(st0[2] - 1.0) <= 1e-15 and abs(st0[3] - 1.0) <= 1e-15  # the start z = 0: r = b
    assert not z.cpu().numpy()[pr.valid].any()


@pytest.mark.parametrize("precond", ["multigrid", "jacobi"])
@pytest.mark.parametrize("name", ["37x41", "33x130"])
def test_check_every_8_reaches_the_same_bound(cuda, name, precond):
    pr = hr.case(name)
    z, _, st = solved(name, precond, "pixel", 8)
    one = solved(name, precond, "pixel", 1)[2]
    assert st[1] == one[1] and st[1] <= st[0] <= st[1] + 7 and (st[0] % 8 == 0 or st[0] == st[1])
    check_solution(pr, z, st)
    assert st[3] <= 10 * RTOL


def test_torch_op_equals_the_python_entry(cuda):
    from rti import ops  # noqa: F401

    pr = hr.case("37x41")
    n = torch.as_tensor(pr.n, device=cuda)
    for jacobi in (False, True):
        ref = solved("37x41", "jacobi" if jacobi else "multigrid", "pixel", 8)[0]
        got = torch.ops.rti.height_from_normals(n, 0.1, False, RTOL, MAX_ITERS, jacobi, None, False, 8)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        got = torch.ops.rti.height_from_normals(n.permute(2, 0, 1).contiguous(), rtol=RTOL, max_iters=MAX_ITERS,
                                                jacobi=jacobi, planar=True)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_into_entry_reuses_a_workspace(cuda):
    pr = hr.case("37x41")
    n = torch.as_tensor(pr.n, device=cuda)
    ws = rti.api.height_workspace(37, 41, "multigrid", cuda)
    ws.fill_(0xFF)  # the workspace need not be initialised: NaN bit patterns everywhere
    z = torch.empty((37, 41), device=cuda)
    st = np.zeros(6)
    for _ in range(2):
        rti.api.height_from_normals_into(n, ws, z, rtol=RTOL, max_iters=MAX_ITERS, check_every=1, stats=st)
        assert np.array_equal(z.cpu().numpy().view(np.uint32), solved("37x41", "multigrid", "pixel")[0].view(np.uint32))
    with pytest.raises(ValueError, match="workspace"):
        rti.api.height_from_normals_into(n, ws[:1024], z)


def test_multigrid_takes_fewer_iterations_than_jacobi(cuda):
    mg, ja = solved("64x64", "multigrid", "pixel")[2], solved("64x64", "jacobi", "pixel")[2]
    assert 0 <= mg[1] < ja[1], (mg, ja)


def test_nz_min_moves_the_mask(cuda):
    pr = hr.Problem(hr.case("37x41").n, nz_min=0.04)
    assert pr.valid.sum() > hr.case("37x41").valid.sum()
    st = np.zeros(6)
    z, v = rti.height_from_normals(torch.as_tensor(pr.n, device=cuda), nz_min=0.04, rtol=RTOL, max_iters=MAX_ITERS,
                                   return_valid=True, stats=st, check_every=1)
    assert np.array_equal(v.cpu().numpy().astype(bool), pr.valid)
    check_solution(pr, z.cpu().numpy(), st)
