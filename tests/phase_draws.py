"""Phase fields with four to eight phases for tests/test_gpu_phase_counts.py (CPU only, deterministic per seed).

pairwise_phases     a matrix and nph - 1 inclusions, at most two non-zero phases per voxel: what the laminate rule accepts
overlapping_phases  smooth fields that overlap, one phase never placed, one below the Voigt threshold: Voigt only.  nph - 2
                    fields are placed, so a voxel holds up to nph - 1 non-zero phases: four and more from nph = 5 on, three at
                    nph = 4 (two placed fields and the tiny phase)
"""
import numpy as np

from helpers import lame


def smooth_field(rng, shape):
    """test_gpu_fuzz.smooth_field: a smooth periodic field in [0, 1] with flat parts at both ends"""
    x = [np.arange(m) / m for m in shape]
    f = np.zeros(shape)
    for _ in range(3):
        k = rng.integers(0, 3, size=3)
        ph = rng.uniform(0, 2 * np.pi, size=3)
        f += rng.uniform(0.5, 1.0) * (np.cos(2 * np.pi * k[0] * x[0] + ph[0])[:, None, None] *
                                      np.cos(2 * np.pi * k[1] * x[1] + ph[1])[None, :, None] *
                                      np.cos(2 * np.pi * k[2] * x[2] + ph[2])[None, None, :])
    f = (f - f.min()) / max(f.max() - f.min(), 1e-300)
    return np.clip(1.6 * f - 0.3, 0.0, 1.0)


def iso_mats(rng, nph):
    """isotropic (mu, lambda) per phase, drawn as the fuzz file draws them"""
    return [lame(E=float(rng.uniform(0.5, 20.0)), nu=float(rng.uniform(0.05, 0.4))) for _ in range(nph)]


def random_normals(rng, shape):
    v = rng.standard_normal((3,) + tuple(shape))
    return v / np.sqrt((v * v).sum(axis=0))


def phase_pairs(phis):
    """{(j, k): number of voxels whose non-zero phases are exactly j < k}, and the largest number of non-zero phases at a voxel"""
    nz = np.stack([p != 0 for p in phis])
    count = nz.sum(axis=0)
    pairs = {}
    for j in range(len(phis)):
        for k in range(j + 1, len(phis)):
            n = int((nz[j] & nz[k] & (count == 2)).sum())
            if n:
                pairs[(j, k)] = n
    return pairs, int(count.max())


def pairwise_phases(grid, nph, rng):
    """(phis, normals).  Phase 0 is the matrix; inclusion k = 1 .. nph-1 lives in the k-th of nph - 1 runs of the voxels in
    storage order, with a smooth profile clipped to exact 0.0 and 1.0, so the supports are disjoint and phi_0 = 1 - phi_k
    there.  Every run holds a pure voxel of its inclusion, a pure matrix voxel and a mixture (0, k).  On the last voxels of
    one run the inclusions j and j + 1 meet with the profiles w and 1 - w exactly and no matrix: the pair (j, j + 1)."""
    grid = tuple(int(v) for v in grid)
    n = grid[0] * grid[1] * grid[2]
    ninc = nph - 1
    assert n >= 6 * ninc, "the grid is too small for %d inclusions" % ninc
    owner = (np.arange(n) * ninc) // n                 # run of every voxel, 0 .. ninc-1
    inc = np.zeros((nph, n))
    for k in range(1, nph):
        run = np.nonzero(owner == k - 1)[0]
        prof = smooth_field(rng, grid).reshape(-1)[run]
        prof[0], prof[1], prof[2] = 1.0, float(rng.uniform(0.1, 0.9)), 0.0   # pure k, a mixture (0, k), pure matrix
        inc[k, run] = prof
    phi0 = 1.0 - inc[1:].sum(axis=0)                   # one non-zero term per voxel: exact
    j = int(rng.integers(1, nph - 1))                  # inclusions j and j + 1 touch
    run = np.nonzero(owner == j - 1)[0]
    layer = run[-max(1, min(grid[2], len(run) // 4)):]
    w = rng.uniform(0.05, 0.95, size=len(layer))
    inc[j, layer] = w
    inc[j + 1, layer] = 1.0 - w
    phi0[layer] = 0.0
    phis = [phi0.reshape(grid)] + [inc[k].reshape(grid) for k in range(1, nph)]
    pairs, deepest = phase_pairs(phis)
    assert deepest == 2, "a voxel holds %d phases" % deepest
    assert len(pairs) >= nph - 1 and all((0, k) in pairs for k in range(1, nph)) and (j, j + 1) in pairs, pairs
    assert all((p == 1).any() for p in phis), "a phase has no pure voxel"
    assert all(((p >= 0) & (p <= 1)).all() for p in phis)
    total = sum(phis)
    assert np.abs(total - 1.0).max() <= 2.3e-16
    return phis, random_normals(rng, grid)


def overlapping_phases(grid, nph, rng):
    """phis for the Voigt rule: smooth fields scaled to sum 1 with voxels of four and more non-zero phases (three at
    nph = 4); phase 2 is zero everywhere (declared, never placed); phase 1 is 5e-16 on a few voxels and zero elsewhere (non-zero, below the 10 eps
    threshold: the skip branch), taken from the matrix there.  The matrix is phase 0 and the other smooth fields are the LAST
    phases, so that a loop that stops short of pt.n loses a phase that matters."""
    grid = tuple(int(v) for v in grid)
    nplaced = nph - 2                                   # phases 0 and 3 .. nph-1 carry the smooth fields
    assert nplaced >= 2
    f = []
    while len(f) < nplaced:
        g = smooth_field(rng, grid)
        if (g > 0).sum() * 4 >= g.size:                 # (a draw of three constant modes is zero everywhere: drawn again)
            f.append(g)
    f[0][sum(f) == 0] = 1.0                             # where nothing was placed: matrix
    total = sum(f)
    phis = [fk / total for fk in f]                     # a voxel only one field reaches is pure: f / f == 1 exactly
    phis[0] = np.where(f[0] > 0, np.maximum(1.0 - sum(phis[1:]), 0.0), 0.0)
    pure = rng.choice(phis[0].size, size=nplaced, replace=False)   # one voxel pure in each placed phase, whatever was drawn
    for k, at in enumerate(pure):
        for q in range(nplaced):
            phis[q].reshape(-1)[at] = 1.0 if q == k else 0.0
    tiny = np.zeros(grid).reshape(-1)
    depth = np.stack([p != 0 for p in phis]).sum(axis=0).reshape(-1)
    rich = np.nonzero((phis[0].reshape(-1) > 0.01) & (phis[0].reshape(-1) < 1))[0]   # matrix that can give 5e-16 away
    rich = rich[np.argsort(-depth[rich], kind="stable")]                             # the deepest mixtures first
    tiny[rich[:max(2, min(len(rich), tiny.size // 50))]] = 5e-16
    tiny = tiny.reshape(grid)
    phis[0] = phis[0] - tiny
    phis = [phis[0], tiny, np.zeros(grid)] + phis[1:]
    assert len(phis) == nph
    assert all((p >= 0).all() for p in phis)
    depth = np.stack([p != 0 for p in phis]).sum(axis=0)
    assert depth.max() >= min(4, nplaced + 1) and (nplaced < 4 or (depth >= 4).any()), depth.max()
    assert not phis[2].any() and 0 < (phis[1] != 0).sum() and phis[1].max() < 10 * np.finfo(float).eps and phis[nph - 1].max() > 0.1
    assert np.abs(sum(phis) - 1.0).max() <= 4 * nph * np.finfo(float).eps
    return phis
