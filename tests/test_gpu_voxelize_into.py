"""LSSolver.voxelize_into (fg_voxelize_into: placed shapes voxelised, normalised and scattered into the solver's padded fields
on the device) against the host path it replaces: geometry.voxelize -> fg._normalize_phi -> set_phase / set_normals.  Both
sides run the same voxeliser kernels on the same inputs and the normalisation is min and subtraction in the same order, so
every comparison is exact."""
import numpy as np
import pytest

from helpers import INCLUSION, MATRIX, lame

pytestmark = pytest.mark.gpu

MATS = [lame(**MATRIX), lame(**INCLUSION), lame(E=4.0, nu=0.25)]


class Fiber:
    def __init__(self, kind, c, a, L, R, material):
        self.kind, self.c, self.a, self.L, self.R, self.material = kind, c, a, L, R, material


def random_capsules(K, seed, materials=(1,)):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(K):
        a = rng.standard_normal(3)
        out.append(Fiber("capsule", rng.random(3).tolist(), a.tolist(), float(rng.uniform(0.0, 0.5)), float(rng.uniform(0.03, 0.12)),
                         int(materials[i % len(materials)])))
    return out


SPHERE = [Fiber("capsule", [.5, .5, .5], [1, 0, 0], 0.0, 0.3, 1)]
HALF_SPACES = [Fiber("halfspace", [0.0, .5, .5], [1, 0, 0], 0, 0.25, 0), Fiber("halfspace", [0.2, .5, .5], [-1, 0, 0], 0, 0.25, 1),
               Fiber("halfspace", [0.5, .5, .5], [-1, 0, 0], 0, 0.25, 2)]
HALF_SPACE_SPHERE = [Fiber("halfspace", [.3, .4, .5], [0.3, -1.0, 0.45], 0, 0.25, 1), Fiber("capsule", [.6, .5, .4], [0, 0, 1], 0.0, 0.2, 1)]
OBLIQUE = [Fiber("capsule", [.1, .4, -.2], [1, 2, -1], 0.7, 0.11, 1)]
OVERLAP = random_capsules(12, 1, (1, 2))
TWO_CAPSULES = [Fiber("capsule", [.45, .5, .5], [1, 1, 0], 0.5, 0.2, 1), Fiber("capsule", [.6, .45, .5], [0, 1, 1], 0.4, 0.22, 2)]

# the smallest grids that reach each layout case: odd nz with a padded tail, nz >= 64 (128-byte row pitch), one row,
# several bricks per axis, an anisotropic cell with an offset origin, overlapping shapes of two materials
CASES = {
    "6x5x7 odd nz": dict(fibers=SPHERE, shape=(6, 5, 7)),
    "8x4x72 pitch": dict(fibers=SPHERE, shape=(8, 4, 72)),
    "10x1x1 half spaces": dict(fibers=HALF_SPACES, shape=(10, 1, 1), nph=3),
    "16x12x20 half space + sphere": dict(fibers=HALF_SPACE_SPHERE, shape=(16, 12, 20)),
    "24x20x36 oblique capsule": dict(fibers=OBLIQUE, shape=(24, 20, 36), dims=(1.0, 2.0, 1.5), x0=(-0.5, -0.6, -1.0)),
    "20^3 overlap, matrix 0": dict(fibers=OVERLAP, shape=(20, 20, 20), nph=3, matrix=0),
    "20^3 overlap, matrix 1": dict(fibers=OVERLAP, shape=(20, 20, 20), nph=3, matrix=1),
    "no shapes": dict(fibers=[], shape=(6, 5, 7), nph=3, matrix=1),
}


def new_solver(shape, dims=(1.0, 1.0, 1.0), nph=2, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*shape, *dims)
    s.set_num_phases(nph)
    for p in range(nph):
        s.set_phase(p, *MATS[p])
    s.set_options(mu_0=2.0, lambda_0=1.5, **opts)   # iterate() takes the reference medium as given
    return s


def host_path(s, fibers, dims=(1.0, 1.0, 1.0), x0=(0.0, 0.0, 0.0), matrix=0, normals=True, **kw):
    """today's hand-over: voxelise to host arrays, normalise in NumPy, upload phase by phase"""
    from fibergen_amd import geometry
    from fibergen_amd.fg import _normalize_phi
    phi, nrm, real = geometry.voxelize(fibers, s.shape, dims, x0, s.nphases, matrix, want_normals=normals, **kw)
    phi = _normalize_phi(phi)
    for p in range(s.nphases):
        s.set_phase(p, *MATS[p], phi[p])
    if normals:
        s.set_normals(nrm)
    return phi, nrm, real


def both(fibers, shape, dims=(1.0, 1.0, 1.0), x0=(0.0, 0.0, 0.0), nph=2, matrix=0, **kw):
    dev, host = new_solver(shape, dims, nph), new_solver(shape, dims, nph)
    real_dev = dev.voxelize_into(fibers, x0, matrix, want_normals=True, **kw)
    phi, nrm, real = host_path(host, fibers, dims, x0, matrix, **kw)
    return dev, host, real_dev, real, phi, nrm


def assert_same_fields(dev, host):
    assert np.array_equal(dev.get_field("phi"), host.get_field("phi"))
    assert np.array_equal(dev.get_field("normals"), host.get_field("normals"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_fields_equal_host_path(name):
    case = dict(CASES[name])
    dev, host, real_dev, real, phi, nrm = both(**case)
    assert_same_fields(dev, host)
    assert np.array_equal(dev.get_field("phi"), phi) and np.array_equal(dev.get_field("normals"), nrm)
    assert real_dev == real   # real_volume equals what geometry.voxelize returns
    for p in range(dev.nphases):
        assert dev.volume_fraction(p) == host.volume_fraction(p)
    if case["fibers"]:
        assert ((phi > 0) & (phi < 1)).any()   # the case has interface voxels
    else:
        m = case["matrix"]
        assert (phi[m] == 1).all() and np.delete(phi, m, axis=0).max() == 0 and np.abs(dev.get_field("normals")).max() == 0
    if name == "20^3 overlap, matrix 0":   # the normalisation acts: the raw fractions of the two materials exceed one somewhere
        from fibergen_amd import geometry
        raw = geometry.voxelize(case["fibers"], case["shape"], (1, 1, 1), (0, 0, 0), 3, case["matrix"])[0]
        assert np.delete(raw, case["matrix"], axis=0).sum(axis=0).max() > 1 + 1e-6


@pytest.mark.parametrize("levels", [-1, 0, 2])
def test_smooth_levels(levels):
    dev, host, real_dev, real, _phi, _nrm = both(OVERLAP, (20, 20, 20), nph=3, smooth_levels=levels)
    assert_same_fields(dev, host)
    assert real_dev == real


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_team_depth_hook(depth):
    from fibergen_amd import _lib
    lib = _lib.load()
    host = new_solver((16, 16, 16))
    host_path(host, SPHERE)
    dev = new_solver((16, 16, 16))
    try:
        lib.fg_voxelize_team_depth(depth)
        dev.voxelize_into(SPHERE, (0, 0, 0), 0, want_normals=True)
    finally:
        lib.fg_voxelize_team_depth(-1)
    assert_same_fields(dev, host)


E = np.array([1.0, 0.2, -0.3, 0.1, 0.0, 0.5])


def test_state_voxelised_twice_then_run_voigt():
    """one solver voxelised twice: the second geometry replaces the first everywhere (moduli, complement test)"""
    shape = (12, 10, 16)
    dev = new_solver(shape, mixing_rule="voigt")
    dev.voxelize_into(SPHERE, (0, 0, 0), 0)
    dev.iterate(E, 1)
    dev.voxelize_into(TWO_CAPSULES[:1], (0, 0, 0), 0)
    host = new_solver(shape, mixing_rule="voigt")
    host_path(host, TWO_CAPSULES[:1], normals=False)
    for s in (dev, host):
        s.set_field("epsilon", np.zeros((6,) + shape))
        s.iterate(E, 3)
    assert np.array_equal(dev.get_field("epsilon"), host.get_field("epsilon"))
    assert np.abs(dev.get_field("epsilon")).max() > 0


def test_state_voxelised_twice_then_run_laminate():
    """laminate mixing: the interface lists are built from device-written phi and normals, rebuilt after the second call"""
    shape = (12, 10, 16)
    dev = new_solver(shape, mixing_rule="laminate")
    dev.voxelize_into(SPHERE, (0, 0, 0), 0, want_normals=True)
    dev.iterate(E, 1)
    dev.voxelize_into(TWO_CAPSULES[:1], (0, 0, 0), 0, want_normals=True)
    host = new_solver(shape, mixing_rule="laminate")
    host_path(host, TWO_CAPSULES[:1])
    for s in (dev, host):
        s.set_field("epsilon", np.zeros((6,) + shape))
        s.iterate(E, 3)
    assert np.array_equal(dev.get_field("epsilon"), host.get_field("epsilon"))
    assert dev.counter("interface_voxels") == host.counter("interface_voxels")
    phi = dev.get_field("phi")
    assert ((phi > 0) & (phi < 1)).any() and np.abs(dev.get_field("normals")).max() > 0   # there are interface voxels to mix


@pytest.mark.parametrize("shape", [(6, 4, 8), (8, 6, 10)])
def test_fine_form_full_staggered(shape):
    """FG_VOX_FINE: the (2n)^3 images are normalised on the device and reduced like set_phase_fine"""
    from fibergen_amd import geometry
    from fibergen_amd.fg import _normalize_phi
    fshape = tuple(2 * n for n in shape)
    dev = new_solver(shape, nph=3, gamma_scheme="full_staggered")
    real_dev = dev.voxelize_into(TWO_CAPSULES, (0, 0, 0), 0, fine=True)
    host = new_solver(shape, nph=3, gamma_scheme="full_staggered")
    raw, _n, real = geometry.voxelize(TWO_CAPSULES, fshape, (1, 1, 1), (0, 0, 0), 3, 0)
    assert (raw[1] + raw[2]).max() > 1 + 1e-6   # the capsules overlap
    fine = _normalize_phi(raw)
    for p in range(3):
        host.set_phase_fine(p, fine[p])
    assert real_dev == real
    assert np.array_equal(dev.get_field("phi"), host.get_field("phi"))
    for s in (dev, host):
        s.iterate(E, 3)
    assert np.array_equal(dev.get_field("epsilon"), host.get_field("epsilon"))
    # a coarse call afterwards clears the fine marks: the solver equals one that never saw a fine image
    dev.voxelize_into(TWO_CAPSULES, (0, 0, 0), 0)
    coarse = new_solver(shape, nph=3, gamma_scheme="full_staggered")
    host_path(coarse, TWO_CAPSULES, normals=False)
    for s in (dev, coarse):
        s.set_field("epsilon", np.zeros((6,) + shape))
        s.iterate(E, 3)
    assert np.array_equal(dev.get_field("epsilon"), coarse.get_field("epsilon"))


def test_phase_uploads_counter():
    dev, host = new_solver((6, 5, 7)), new_solver((6, 5, 7))
    dev.voxelize_into(SPHERE, (0, 0, 0), 0, want_normals=True)
    host_path(host, SPHERE)
    assert dev.counter("phase_uploads") == 0
    assert host.counter("phase_uploads") == 3   # two phases and the normals


def test_errors():
    s = new_solver((4, 4, 4))
    with pytest.raises(RuntimeError, match="material out of range"):
        s.voxelize_into([Fiber("capsule", [.5, .5, .5], [1, 0, 0], 0.0, 0.3, 2)], (0, 0, 0), 0)
    with pytest.raises(RuntimeError, match="zero normal"):
        s.voxelize_into([Fiber("halfspace", [0, 0, 0], [0, 0, 0], 0, 0.1, 1)], (0, 0, 0), 0)
    with pytest.raises(RuntimeError, match="orientation"):
        s.voxelize_into([Fiber("capsule", [0, 0, 0], [0, 0, 0], 0.5, 0.1, 1)], (0, 0, 0), 0)
    with pytest.raises(RuntimeError, match="needs gamma_scheme full_staggered"):
        s.voxelize_into(SPHERE, (0, 0, 0), 0, fine=True)
    assert s.counter("phase_uploads") == 0 and np.abs(s.get_field("phi")).max() == 0   # nothing was written
    from fibergen_amd.distributed import SlabMember
    slab = SlabMember(4, 4, 4, rank=0, nranks=1)
    slab.set_num_phases(2)
    with pytest.raises(RuntimeError, match="slab-decomposed"):
        slab.voxelize_into(SPHERE, (0, 0, 0), 0)
