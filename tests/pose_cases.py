"""The inputs of the pose gradient tests, in numpy alone, so that tests/test_pose_ref.py (CPU) checks the power of the bound on
exactly the cases tests/test_pose_grad_gpu.py runs on the GPU.

N_OPS restates the count of gsrt_pose_grad.hip's header: the longest chain of rounded float32 operations from the kernel's
inputs to one of a Gaussian's 16 contributions. It is k_splat_grad_to_model's chain up to dL/dt (tests/test_geom_grad_gpu.py's
CHAIN_OPS = 37 less the final MV^T dL/dt, 4 operations: 33), then gt[r] * c4[c] (1) and the sum with the direct term (1): 35;
the depth form subtracts row[6] first: 36.
"""
import numpy as np

import cor_f64_pose as PQ
import oracle as O

N_OPS = {False: 33 + 2, True: 34 + 2}
EPS = 2.0 ** -24
CHUNK, LANES = 2048, 512  # what gsrt_debug_pose_grad_layout reports; both tests assert it
W, H = 64, 48


def seam_sizes(chunk=CHUNK, lanes=LANES):
    """(n, starred): the sizes at which the kernels take another path; the starred ones run both depth forms"""
    return [(1, False), (63, False), (64, True), (65, False), (255, False), (256, False), (257, False), (chunk - 1, False),
            (chunk, True), (chunk + 1, False), (3 * chunk + 17, False), (lanes * chunk + 1, True)]


def seam_cases():
    return [(n, d) for n, star in seam_sizes() for d in ((False, True) if star else (False,))]


def camera(mv=None, projection=None):
    ubo = O.make_ubo(O.lookat((0.1, -0.05, 0.2), (0.0, 0.05, -1.0)) if mv is None else mv, 60.0, W, H, 1.0, 1, 16)
    if projection is not None:
        ubo["projection"][0] = np.asarray(projection, np.float32).reshape(16)
    return ubo


def nonaffine_camera():
    """a model-view whose bottom row is not (0, 0, 0, 1), and a general projection (every entry non-zero where the kernel
    reads it: rows 0, 1 and 3)"""
    ubo = camera()
    mv = ubo["model_view"][0].copy().reshape(4, 4)  # [c][r]
    mv[:, 3] += np.array([0.02, -0.03, 0.01, 0.05], np.float32)
    ubo["model_view"][0] = mv.reshape(16)
    ubo["model_view_inverse"][0] = np.linalg.inv(mv.astype(np.float64)).astype(np.float32).reshape(16)  # [c][r] both ways
    P =ubo["projection"][0].copy().reshape(4, 4)
    P[:, 0] += np.array([0.0, 0.05, -0.04, 0.03], np.float32)
    P[:, 1] += np.array([0.06, 0.0, 0.02, -0.05], np.float32)
    P[:, 3] += np.array([0.01, -0.02, 0.0, 0.04], np.float32)
    ubo["projection"][0] = P.reshape(16)
    return ubo


def synthetic(n, seed, ubo=None):
    """params (n, 12), aabbs (n, 6), rows (n, 8), behind (n,) bool, all float32: centres in the frustum 2..8 in front of
    the camera, random positive definite covariances, normal rows; every Gaussian with index % 6 == 5 stands behind the
    camera and has a row of ones"""
    ubo = camera() if ubo is None else ubo
    rng = np.random.default_rng(seed)
    z = -rng.uniform(2.0, 8.0, n)
    behind = np.arange(n) % 6 == 5
    z[behind] = rng.uniform(1.0, 3.0, int(behind.sum()))
    view = np.stack([rng.uniform(-0.5, 0.5, n) * np.abs(z), rng.uniform(-0.4, 0.4, n) * np.abs(z), z, np.ones(n)], -1)
    inv = np.linalg.inv(PQ.mat(ubo["model_view"][0]))
    world = view @ inv.T
    world = world[:, :3] / world[:, 3:4]
    A = rng.normal(0.0, 0.08, (n, 3, 3))
    S = A @ np.transpose(A, (0, 2, 1)) + 4e-4 * np.eye(3)
    params = np.zeros((n, 12), np.float32)
    params[:, :3] = world
    params[:, 3] = rng.uniform(0.1, 1.0, n)
    params[:, 4:10] = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
    rad = 3.0 * np.sqrt(np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2]], -1))
    aabbs = np.concatenate([params[:, :3] - rad, params[:, :3] + rad], 1).astype(np.float32)
    rows = rng.normal(0.0, 1.0, (n, 8)).astype(np.float32)
    rows[:, 7] = 0.0
    rows[behind] = 1.0
    return params, aabbs, rows, behind


def reference(ubo, params, rows, depth, fault=None, step=1 << 16):
    """(G, bound, valid): pose_chain of float32 parameters and rows, taken over chunks of `step` Gaussians so that the
    (n, 4, 4) arrays of the largest case stay small; bound as cor_f64_pose.bound defines it"""
    n = len(params)
    G, B = np.zeros((4, 4)), np.zeros((4, 4))
    valid = np.zeros(n, bool)
    for a in range(0, n, step):
        p = params[a:a + step].astype(np.float64)
        ref = PQ.pose_chain(ubo, p[:, :3], p[:, 4:10], rows[a:a + step].astype(np.float64), depth, fault)
        G += ref.G
        B += (N_OPS[depth] * (1.0 + ref.kappa)[:, None, None] * EPS * ref.Mg).sum(0)
        valid[a:a + step] = ref.valid
    return G, B + EPS * np.abs(G), valid
