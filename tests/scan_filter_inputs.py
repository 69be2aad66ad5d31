"""Inputs of the lcd_filter_scans tests: the hand-made scans of every branch of the rule and the batches of the GPU tests.
tests/test_scan_filter_inputs.py proves with tests/scan_filter_model.py that each case does what it is named for."""
import numpy as np

F = np.float32
SIZES = (0, 1, 2, 3, 4, 5, 6, 255, 256, 257, 511, 512, 513)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cloud(n, seed, span=1.0):
    return np.random.default_rng(seed).uniform(-span, span, (n, 3)).astype(np.float32)


def lattice(nx, ny, nz, spacing=1.0, origin=(0.0, 0.0, 0.0)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), axis=-1).reshape(-1, 3)
    return (g * spacing + np.asarray(origin)).astype(np.float32)


def size_batch():
    """every size of SIZES with an empty scan behind each"""
    scans = []
    for k, n in enumerate(SIZES):
        scans += [cloud(n, 100 + k), np.zeros((0, 3), np.float32)]
    return scans


def runs(lengths, leaf=0.5):
    """voxel i along x holds lengths[i] rows, shuffled so that a voxel's rows are not neighbours in the scan"""
    rng = np.random.default_rng(5)
    rows = [np.column_stack([rng.uniform(i * leaf + 0.01, (i + 1) * leaf - 0.01, n), rng.uniform(0.01, leaf - 0.01, (n, 2))]) for i, n in enumerate(lengths)]
    x = np.concatenate(rows)
    return x[rng.permutation(len(x))].astype(np.float32)


def on_the_bounds():
    """(3, 4, 0) has r = 25 exactly; beside it the nearest x below and above 3 whose r leaves 25; the last row only stays with is_2d"""
    lo, hi = F(3), F(3)
    while lo * lo + F(16) >= F(25):
        lo = np.nextafter(lo, F(0))
    while hi * hi + F(16) <= F(25):
        hi = np.nextafter(hi, F(9))
    return np.array([[3, 4, 0], [lo, 4, 0], [hi, 4, 0], [0, 0, 5], [1, 1, 1], [6, 8, 0], [3, 4, 100]], np.float32)


def tilted_plane():
    """a plane with the normal (0.6, 0, -0.8) around x = -20 that spans z = 9 .. 11: seen from (0, 0, 10) no normal points away, so only the
    ground rule's second condition can turn one, and only below z = 10"""
    rng = np.random.default_rng(9)
    s, t = rng.uniform(-1.25, 1.25, 400), rng.uniform(-1, 1, 400)
    return (np.array([-20.0, 0, 10.0]) + s[:, None] * np.array([0.8, 0, 0.6]) + t[:, None] * np.array([0, 1.0, 0])).astype(np.float32)


def ground_edge(M):
    """-> (scan, kw, up_equal, up_below): with ground_normals_up = up_equal some row's n_z equals -up exactly (not turned), with up_below the
    same n_z lies just below -up (turned when p_z < 10)"""
    scan = tilted_plane()
    kw = dict(normal_k=8)
    r = M.filter_scan(scan, **kw)
    nz = r["normals"][:r["count"], 2]
    pz = r["xyz"][:r["count"], 2]
    row = int(np.flatnonzero((nz < 0) & (pz < 10))[0])
    up = -nz[row]
    return scan, kw, float(up), float(np.nextafter(up, F(0)))


def cases():
    """name -> dict(scans, caps (None: each scan's own size), kw, device_only)"""
    c = {}

    def add(name, scans, caps=None, device_only=False, **kw):
        c[name] = dict(scans=[np.ascontiguousarray(s, np.float32).reshape(-1, 3) for s in scans], caps=caps, kw=kw, device_only=device_only)

    big = cloud(40, 1)
    add("step_2", [cloud(2, 2), cloud(3, 3), big], downsampling_step=2)
    add("step_3", [cloud(3, 4), cloud(4, 5), big], downsampling_step=3)
    add("range_min", [on_the_bounds()], range_min=5.0)
    add("range_max", [on_the_bounds()], range_max=5.0)
    add("range_both", [on_the_bounds(), big * 6], range_min=5.0, range_max=10.0)
    add("range_negative_min", [on_the_bounds()], range_min=-1.0, range_max=5.0)
    add("range_2d", [on_the_bounds()], range_max=5.0, is_2d=True)
    bad = cloud(300, 6)
    bad[[0, 255, 256], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    add("not_finite_rows", [bad, bad], device_only=True, downsampling_step=2)
    add("not_finite_rows_voxel_normals", [bad], device_only=True, voxel_size=0.2, normal_k=5, range_max=10.0)
    add("one_voxel_513", [np.random.default_rng(7).uniform(0.01, 0.09, (513, 3))], voxel_size=0.1)
    add("every_row_its_voxel", [lattice(9, 8, 7)], voxel_size=0.5)
    add("runs", [runs((1, 2, 255, 256, 257))], voxel_size=0.5)
    add("negative_coordinates", [cloud(300, 8) - F(3)], voxel_size=0.3)
    add("multiples_of_the_leaf", [lattice(6, 5, 4, 0.25, (-0.75, -0.5, 0.0))], voxel_size=0.25)
    add("grid_too_large", [np.array([[0, 0, 0], [1e4, 1e4, 1e4]]), big], voxel_size=0.01)
    add("cell_beyond_int32", [np.array([[0, 0, 0], [3e9, 0, 0]]), big], voxel_size=1.0)
    room = cloud(300, 10)
    for k in (1, 2, 3, 5, 8, 9, 16, 17, 32):
        add("k_%d" % k, [room, cloud(4, 11), cloud(2, 12)], normal_k=k)
    add("k_lattice_ties", [lattice(5, 5, 4)], normal_k=5)
    add("k_duplicates", [np.repeat(cloud(60, 13), 3, axis=0)], normal_k=5)
    add("k_collinear", [np.column_stack([np.arange(20.0), 2 * np.arange(20.0), np.zeros(20)]) + 1], normal_k=5)
    add("k_flat_z0", [lattice(8, 8, 1, 1.0, (-3.0, -4.0, 0.0))], normal_k=9)
    add("radius_lattice", [lattice(5, 5, 4)], normal_radius=1.0)
    add("radius_sparse", [cloud(200, 14, 3.0)], normal_radius=0.6)
    add("voxel_then_normals", [cloud(600, 15), cloud(513, 16)], voxel_size=0.25, normal_k=5, viewpoint=(0.5, -0.25, 2.0))
    add("ground_up", [tilted_plane(), lattice(8, 8, 1, 0.5, (-2.0, -2.0, 12.0))], normal_k=8, ground_normals_up=0.5)
    fit = lattice(4, 4, 4)
    add("capacity_exact", [fit, fit], caps=[64, 64], voxel_size=0.5)
    add("capacity_one_short", [fit, fit], caps=[63, 64], voxel_size=0.5)
    add("capacity_one_short_normals", [fit, fit], caps=[64, 63], normal_k=5)
    add("capacity_zero", [fit], caps=[0], normal_k=5)
    add("larger_region", [room], caps=[1024], voxel_size=0.2, normal_k=5)
    return c


def spread(n, seed):
    """n points over a box wide enough that a leaf of 0.05 merges few of them"""
    return np.random.default_rng(seed).uniform(-4, 4, (n, 3)).astype(np.float32)


def concatenate(scans, caps=None):
    """-> xyz [N x 3], offsets, out_offsets"""
    z = np.zeros((0, 3), np.float32)
    n = [s.shape[0] for s in scans]
    caps = n if caps is None else caps
    return (np.concatenate(list(scans) + [z]), np.concatenate([[0], np.cumsum(n)]).astype(np.int64), np.concatenate([[0], np.cumsum(caps)]).astype(np.int64))
