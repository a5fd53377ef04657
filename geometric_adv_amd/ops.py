"""The reference's operator API for the attack path, on MI355X.

Function names, argument order and output order are those of the reference's Python wrappers
(external/structural_losses/tf_nndistance.py:15-41, tf_approxmatch.py:10-50,
external/grouping/tf_grouping.py:8-75).  Inputs and outputs are torch tensors on an AMD GPU
(containers only: the arithmetic runs in libgeoadv.so's hand-written gfx950 kernels).
Shape errors raise ValueError (the reference raises InvalidArgumentError from OP_REQUIRES).
"""
import ctypes as C

import torch

from . import _abi, _lib
from ._abi import BatchAugment, CloudAugment    # noqa: F401  -- part of this module's interface


def _f32(t, name, rank):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got %s); there is no CPU path" % (name, t.device))
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32 (got %s)" % (name, t.dtype))
    if t.dim() != rank:
        raise ValueError("%s must have rank %d (got shape %s)" % (name, rank, tuple(t.shape)))
    return t.contiguous()


def _i32(t, name, shape):
    if not t.is_cuda or t.dtype != torch.int32:
        raise ValueError("%s must be an int32 GPU tensor" % name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be of shape %s (got %s)" % (name, tuple(shape), tuple(t.shape)))
    return t.contiguous()


def _xyz_pair(xyz1, xyz2, op):
    xyz1 = _f32(xyz1, "xyz1", 3)
    xyz2 = _f32(xyz2, "xyz2", 3)
    if xyz1.shape[2] != 3:
        raise ValueError("%s only accepts 3d point set xyz1" % op)          # tf_nndistance.cpp:52
    if xyz2.shape[2] != 3:
        raise ValueError("%s only accepts 3d point set xyz2" % op)          # tf_nndistance.cpp:56
    if xyz1.shape[0] != xyz2.shape[0]:
        raise ValueError("%s expects xyz1 and xyz2 have same batch size" % op)  # tf_nndistance.cpp:58
    return xyz1, xyz2


NN_SYM_MIN_PAIRS = 1 << 26      # b * n * m from which nn_distance(kernel="auto") takes the symmetric scan (measured, tools/debug/nn_op_time.py:
                                # 32 x 2048 x 2048: 0.050 -> 0.039 ms, 256 x 2048 x 2048: 0.35 -> 0.22, 32 x 8192 x 8192: 0.62 -> 0.37; smaller
                                # problems are host-bound either way and keep the one-launch kernel)


def nn_distance(xyz1, xyz2, kernel="auto"):
    """tf_nndistance.py:15-26.  xyz1 (b,n,3), xyz2 (b,m,3) ->
    dist1 (b,n) squared distance from each xyz1 point to its nearest xyz2 point, idx1 (b,n) int32,
    dist2 (b,m), idx2 (b,m).  Bit-identical to the reference CPU op; lowest index wins ties.
    kernel: "scan" = the reference-shaped entry point geoadv_nn_distance (two scans, no scratch), "symmetric" = every pair distance
    once for both directions (nn_distance_sym: the attack loop's kernel, scratch from torch), "auto" = by size.  Same bits."""
    if kernel not in ("auto", "scan", "symmetric"):
        raise ValueError("kernel must be 'auto', 'scan' or 'symmetric'")
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "NnDistance")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if n >= 1 and m >= 1 and b >= 1 and (kernel == "symmetric" or (kernel == "auto" and b * n * m >= NN_SYM_MIN_PAIRS)):
        return nn_distance_sym(xyz1, xyz2)
    dist1 = torch.empty((b, n), dtype=torch.float32, device=xyz1.device)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=xyz1.device)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=xyz1.device)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        st = _lib.lib().geoadv_nn_distance(b, n, _lib.ptr(xyz1), m, _lib.ptr(xyz2), _lib.ptr(dist1), _lib.ptr(idx1),
                                           _lib.ptr(dist2), _lib.ptr(idx2), _lib.stream_handle())
    _lib.check(st, "nn_distance")
    return dist1, idx1, dist2, idx2


def chamfer_screen(on):
    """Process-wide switch of the matrix-pipe-screened symmetric scan (csrc/chamfer_mx.h; default on): False = the unscreened scan
    everywhere.  Same results either way, bit for bit; returns the previous setting."""
    return bool(_lib.lib().geoadv_set_chamfer_screen(1 if on else 0))


def nn_distance_sym(xyz1, xyz2):
    """nn_distance with every pair distance evaluated ONCE for both directions (the attack loop's kernel): identical outputs,
    bit for bit; both clouds need at least one point."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "NnDistance")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if n < 1 or m < 1:
        raise ValueError("nn_distance_sym needs non-empty clouds")
    dist1 = torch.empty((b, n), dtype=torch.float32, device=xyz1.device)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=xyz1.device)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=xyz1.device)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=xyz1.device)
    wf = int(_lib.lib().geoadv_nn_distance_sym_workspace_floats(b, n, m))
    ws = torch.empty((wf,), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        st = _lib.lib().geoadv_nn_distance_sym(b, n, _lib.ptr(xyz1), m, _lib.ptr(xyz2), _lib.ptr(dist1), _lib.ptr(idx1),
                                               _lib.ptr(dist2), _lib.ptr(idx2), _lib.ptr(ws), wf, _lib.stream_handle())
    _lib.check(st, "nn_distance_sym")
    return dist1, idx1, dist2, idx2


def nn_distance_lists(xyz1_anchor, xyz2, dist1_anchor, dist2_anchor, skin, xyz1, capacity=16):
    """nn_distance(xyz1, xyz2) from exact neighbour lists (csrc/chamfer_lists.hip: what the attack loop does between two all-pairs
    scans of (recon, target)): the lists are built from the anchor cloud xyz1_anchor, its exact minima against xyz2 and a skin per
    cloud (scalar or (b,)), then queried with the moved xyz1.  Returns (dist1, idx1, dist2, idx2, state, flags): the four outputs of
    nn_distance(xyz1, xyz2) bit for bit; state int64 (3,): queries certified from their list, listed but refused, unlisted (the
    last two are answered by brute force in the same launch); flags int32 (b,): clouds the loop would hand back to the scan."""
    xyz1_anchor, xyz2 = _xyz_pair(xyz1_anchor, xyz2, "NnDistanceLists")
    xyz1 = _f32(xyz1, "xyz1", 3)
    if tuple(xyz1.shape) != tuple(xyz1_anchor.shape):
        raise ValueError("nn_distance_lists expects xyz1 of the anchor's shape")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dev = xyz1.device
    d1a, d2a = _f32(dist1_anchor, "dist1_anchor", 2), _f32(dist2_anchor, "dist2_anchor", 2)
    if tuple(d1a.shape) != (b, n) or tuple(d2a.shape) != (b, m):
        raise ValueError("nn_distance_lists expects the anchor minima as (b, n) and (b, m)")
    sk = torch.as_tensor(skin, dtype=torch.float32, device=dev).reshape(-1)
    sk = (sk.expand(b) if sk.numel() == 1 else sk).contiguous()
    if sk.numel() != b:
        raise ValueError("nn_distance_lists expects one skin, or one per cloud")
    dist1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    state = torch.zeros((4,), dtype=torch.int64, device=dev)
    flags = torch.zeros((b,), dtype=torch.int32, device=dev)
    wb = int(_lib.lib().geoadv_nn_distance_lists_workspace_bytes(b, n, m, int(capacity)))
    ws = torch.empty((wb,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        st = _lib.lib().geoadv_nn_distance_lists(b, n, m, _lib.ptr(xyz1_anchor), _lib.ptr(xyz2), _lib.ptr(d1a), _lib.ptr(d2a),
                                                 _lib.ptr(sk), int(capacity), _lib.ptr(xyz1), _lib.ptr(dist1), _lib.ptr(idx1),
                                                 _lib.ptr(dist2), _lib.ptr(idx2), _lib.ptr(state), _lib.ptr(flags), _lib.ptr(ws), wb,
                                                 _lib.stream_handle())
    _lib.check(st, "nn_distance_lists")
    return dist1, idx1, dist2, idx2, state[:3], flags


def chamfer_per_pc(dist1, dist2):
    """tf.reduce_mean(dist1, axis=1) + tf.reduce_mean(dist2, axis=1) of nn_distance's outputs (adv_ae.py:121,132;
    get_dists_per_point.py:75): (b,n), (b,m) -> (b,).  Summation order = the attack loop's own metrics, so a Chamfer
    distance recomputed from saved clouds is bit-identical to adversarial_metrics[:, :, 2]."""
    dist1, dist2 = _f32(dist1, "dist1", 2), _f32(dist2, "dist2", 2)
    if dist1.shape[0] != dist2.shape[0]:
        raise ValueError("chamfer_per_pc expects dist1 and dist2 have same batch size")
    b, n = dist1.shape
    m = dist2.shape[1]
    out = torch.empty((b,), dtype=torch.float32, device=dist1.device)
    with torch.cuda.device(dist1.device):
        st = _lib.lib().geoadv_chamfer_per_pc(b, n, m, _lib.ptr(dist1), _lib.ptr(dist2), _lib.ptr(out), _lib.stream_handle())
    _lib.check(st, "chamfer_per_pc")
    return out


def nn_distance_paired(xyz1, xyz2):
    """nn_distance for paired clouds of equal size (xyz1[j] close to xyz2[j] for most j, like adv = x + pert): exact
    grid search seeded with the pairing; identical results, fast when the pairing is good."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "NnDistance")
    b, n, _ = xyz1.shape
    if xyz2.shape[1] != n:
        raise ValueError("nn_distance_paired needs clouds of equal size")
    dist1 = torch.empty((b, n), dtype=torch.float32, device=xyz1.device)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=xyz1.device)
    dist2, idx2 = torch.empty_like(dist1), torch.empty_like(idx1)
    with torch.cuda.device(xyz1.device):
        st = _lib.lib().geoadv_nn_distance_paired(b, n, _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(dist1), _lib.ptr(idx1),
                                                  _lib.ptr(dist2), _lib.ptr(idx2), _lib.stream_handle())
    _lib.check(st, "nn_distance_paired")
    return dist1, idx1, dist2, idx2


def nn_distance_grad(xyz1, xyz2, grad_dist1, idx1, grad_dist2, idx2):
    """The NnDistanceGrad op behind tf_nndistance.py:35-41 -> (grad_xyz1, grad_xyz2)."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "NnDistanceGrad")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    grad_dist1 = _f32(grad_dist1, "grad_dist1", 2)
    grad_dist2 = _f32(grad_dist2, "grad_dist2", 2)
    if tuple(grad_dist1.shape) != (b, n):
        raise ValueError("NnDistanceGrad requires grad_dist1 be of shape(batch,#points)")   # tf_nndistance.cpp:102
    if tuple(grad_dist2.shape) != (b, m):
        raise ValueError("NnDistanceGrad requires grad_dist2 be of shape(batch,#points)")   # tf_nndistance.cpp:104
    idx1 = _i32(idx1, "idx1", (b, n))
    idx2 = _i32(idx2, "idx2", (b, m))
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    with torch.cuda.device(xyz1.device):
        st = _lib.lib().geoadv_nn_distance_grad(b, n, _lib.ptr(xyz1), m, _lib.ptr(xyz2), _lib.ptr(grad_dist1),
                                                _lib.ptr(idx1), _lib.ptr(grad_dist2), _lib.ptr(idx2), _lib.ptr(g1),
                                                _lib.ptr(g2), _lib.stream_handle())
    _lib.check(st, "nn_distance_grad")
    return g1, g2


class _NnDistanceFn(torch.autograd.Function):
    """Autograd glue equivalent to @ops.RegisterGradient('NnDistance') (tf_nndistance.py:35-41)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        d1, i1, d2, i2 = nn_distance(xyz1, xyz2)
        ctx.save_for_backward(xyz1, xyz2, i1, i2)
        ctx.mark_non_differentiable(i1, i2)
        return d1, i1, d2, i2

    @staticmethod
    def backward(ctx, gd1, _gi1, gd2, _gi2):
        xyz1, xyz2, i1, i2 = ctx.saved_tensors
        g1, g2 = nn_distance_grad(xyz1, xyz2, gd1.contiguous(), i1, gd2.contiguous(), i2)
        return g1, g2


def nn_distance_autograd(xyz1, xyz2):
    """nn_distance with the registered gradient, for callers that differentiate through it."""
    return _NnDistanceFn.apply(xyz1, xyz2)


# ---------------------------------------------------------------------------------------------
# external/grouping/tf_grouping.py
# ---------------------------------------------------------------------------------------------
def _call(name, *args):
    st = getattr(_lib.lib(), name)(*args, _lib.stream_handle())
    _lib.check(st, name.replace("geoadv_", ""))


def query_ball_point(radius, nsample, xyz1, xyz2):
    """tf_grouping.py:8-20.  xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries ->
    idx (b,m,nsample) int32 (first nsample points within radius, padded with the first hit),
    pts_cnt (b,m) int32."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "QueryBallPoint")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    idx = torch.zeros((b, m, int(nsample)), dtype=torch.int32, device=xyz1.device)
    cnt = torch.zeros((b, m), dtype=torch.int32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        _call("geoadv_query_ball_point", b, n, m, float(radius), int(nsample), _lib.ptr(xyz1), _lib.ptr(xyz2),
              _lib.ptr(idx), _lib.ptr(cnt))
    return idx, cnt


def select_top_k(k, dist):
    """tf_grouping.py:22-31.  dist (b,m,n) -> idx (b,m,n) int32, dist_out (b,m,n); the first k
    entries of every row are the k smallest in ascending order (the reference's swap order)."""
    dist = _f32(dist, "dist", 3)
    b, m, n = dist.shape
    outi = torch.empty((b, m, n), dtype=torch.int32, device=dist.device)
    out = torch.empty_like(dist)
    with torch.cuda.device(dist.device):
        _call("geoadv_selection_sort", b, n, m, int(k), _lib.ptr(dist), _lib.ptr(outi), _lib.ptr(out))
    return outi, out


def group_point(points, idx):
    """tf_grouping.py:33-41.  points (b,n,c), idx (b,m,nsample) -> out (b,m,nsample,c)."""
    points = _f32(points, "points", 3)
    b, n, c = points.shape
    if idx.dim() != 3 or idx.shape[0] != b:
        raise ValueError("GroupPoint expects idx of shape (batch, npoint, nsample)")
    idx = _i32(idx, "idx", idx.shape)
    m, ns = idx.shape[1], idx.shape[2]
    out = torch.empty((b, m, ns, c), dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _call("geoadv_group_point", b, n, c, m, ns, _lib.ptr(points), _lib.ptr(idx), _lib.ptr(out))
    return out


def group_point_grad(points, idx, grad_out):
    """The GroupPointGrad op behind tf_grouping.py:42-46 -> grad_points (b,n,c)."""
    points = _f32(points, "points", 3)
    b, n, c = points.shape
    idx = _i32(idx, "idx", idx.shape)
    m, ns = idx.shape[1], idx.shape[2]
    grad_out = _f32(grad_out, "grad_out", 4)
    if tuple(grad_out.shape) != (b, m, ns, c):
        raise ValueError("GroupPointGrad expects grad_out of shape (batch, npoint, nsample, channel)")
    gp = torch.empty_like(points)
    with torch.cuda.device(points.device):
        wb = int(_lib.lib().geoadv_group_point_grad_workspace_bytes(b, n, c, m, ns))
        ws = torch.empty(wb, dtype=torch.uint8, device=points.device)       # caller-owned scratch (torch's caching allocator)
        _call("geoadv_group_point_grad_ws", b, n, c, m, ns, _lib.ptr(grad_out), _lib.ptr(idx), _lib.ptr(gp), _lib.ptr(ws), wb)
    return gp


KNN_KERNELS = {"auto": _abi.GEOADV_KNN_AUTO, "all_points": _abi.GEOADV_KNN_ALL_POINTS, "grid": _abi.GEOADV_KNN_GRID,
               "grid_shells": _abi.GEOADV_KNN_GRID_SHELLS}
_knn_default = "auto"


def _knn_kernel(kernel):
    k = _knn_default if kernel is None else kernel
    if k not in KNN_KERNELS:
        raise ValueError("kernel must be one of %s" % sorted(KNN_KERNELS))
    return KNN_KERNELS[k]


def knn_point(k, xyz1, xyz2, kernel=None):
    """tf_grouping.py:48-75.  xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> val (b,m,k) squared
    distances ascending, idx (b,m,k) int32 -- fused (no (b,m,n) matrix), same order among equal
    distances as the reference's SelectionSort.
    kernel: which kernel answers THIS call -- "auto" (by size), "all_points", "grid", "grid_shells" (same results; None = the
    default set by knn_grid_mode).  The scratch is a torch tensor (caller-owned workspace of the C ABI's _ws form)."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "knn_point")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    val = torch.empty((b, m, int(k)), dtype=torch.float32, device=xyz1.device)
    idx = torch.empty((b, m, int(k)), dtype=torch.int32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        wb = int(_lib.lib().geoadv_knn_workspace_bytes(b, n, m, int(k)))
        ws = torch.empty(wb, dtype=torch.uint8, device=xyz1.device)
        _call("geoadv_knn_point_ws", _knn_kernel(kernel), b, n, m, int(k), _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(val), _lib.ptr(idx),
              _lib.ptr(ws), wb)
    return val, idx


def knn_grid_mode(mode):
    """TESTS / MEASUREMENTS: the default k-NN kernel of this module's calls that pass no `kernel` ("auto" by size, "all_points",
    "grid", "grid_shells" = the grid search without its lane-private first pass) -- and of the C ABI's reference-shaped entry
    points (geoadv_knn_grid_mode).  Concurrent callers pass `kernel=` per call instead."""
    global _knn_default
    if mode not in KNN_KERNELS:
        raise ValueError("mode must be one of %s" % sorted(KNN_KERNELS))
    _lib.check(_lib.lib().geoadv_knn_grid_mode(KNN_KERNELS[mode]), "knn_grid_mode")
    _knn_default = mode


def knn_dists(pc, num_knn, kernel=None):
    """The graph of defender/get_knn_dists_per_point.py:78-81 fused: distances (not squared) from
    every point to its num_knn nearest neighbours, self dropped.  pc (b,n,3) -> (b,n,num_knn).  kernel: as knn_point."""
    pc = _f32(pc, "pc", 3)
    if pc.shape[2] != 3:
        raise ValueError("knn_dists only accepts 3d point sets")
    b, n, _ = pc.shape
    out = torch.empty((b, n, int(num_knn)), dtype=torch.float32, device=pc.device)
    with torch.cuda.device(pc.device):
        wb = int(_lib.lib().geoadv_knn_workspace_bytes(b, n, n, int(num_knn) + 1))
        ws = torch.empty(wb, dtype=torch.uint8, device=pc.device)
        _call("geoadv_knn_dists_ws", _knn_kernel(kernel), b, n, int(num_knn), _lib.ptr(pc), _lib.ptr(out), _lib.ptr(ws), wb)
    return out


FPS_MAX_POINTS = 16384                                      # include/geoadv.h geoadv_farthest_point_sample
FPS_FORMS = {"auto": _abi.GEOADV_FPS_AUTO, "workgroup": _abi.GEOADV_FPS_WORKGROUP, "wave": _abi.GEOADV_FPS_WAVE}


def _fps_form(form):
    if form not in FPS_FORMS:
        raise ValueError("form must be one of %s" % sorted(FPS_FORMS))
    return FPS_FORMS[form]


def farthest_point_sample_plan(n, form="auto"):
    """The kernel instance that answers a cloud of n points (geoadv_farthest_point_sample_plan; no launch, no device) ->
    (form "workgroup" or "wave", waves that share a cloud, points per thread).  ValueError where the op refuses (n, form)."""
    f, w, p = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().geoadv_farthest_point_sample_plan(int(n), _fps_form(form), C.byref(f), C.byref(w), C.byref(p)),
               "farthest_point_sample_plan")
    return {1: "workgroup", 2: "wave"}[f.value], w.value, p.value


def _fps_start(start, b, n, dev):
    """start of farthest_point_sample -> None or an int32 device tensor (b,) with every value outside [0, n) read as 0."""
    import numpy as np
    if start is None:
        return None
    if isinstance(start, torch.Tensor):
        if start.dim() != 1 or start.shape[0] != b or start.dtype not in (torch.int32, torch.int64):
            raise ValueError("start must be an int, or an int32 or int64 tensor of shape (%d,); got %s of shape %s" % (b, start.dtype, tuple(start.shape)))
        s = start.to(dev)
        return torch.where((s >= 0) & (s < n), s, torch.zeros_like(s)).to(torch.int32).contiguous()
    if isinstance(start, (int, np.integer)) and not isinstance(start, bool):
        host = np.full((b,), int(start), dtype=np.int64)
    else:
        host = np.asarray(start)
        if host.shape != (b,) or host.dtype.kind not in "iu":
            raise ValueError("start must be an int, or an integer array of shape (%d,)" % b)
        host = host.astype(np.int64)
    return torch.from_numpy(np.where((host >= 0) & (host < n), host, 0).astype(np.int32)).to(dev)


def farthest_point_sample(xyz, npoint, start=None, return_points=False, return_mindist=False, form="auto"):
    """Farthest point sampling (csrc/sampling.hip, the rule in include/geoadv.h): xyz (b,n,3) -> idx (b,npoint) int32, per cloud
    the start index and then, npoint - 1 times, the point with the largest squared distance to those chosen so far (fp32, the
    lowest index among equals).  npoint == n on distinct finite points is the cloud in farthest-point order.  A point with a NaN
    or infinite coordinate is never chosen (except as the given start); 1 <= npoint <= n <= 16384.
    start: None (index 0), an int for every cloud, or a (b,) int32 / int64 tensor or integer array; a value outside [0, n) reads as 0.
    return_points: also sampled (b,npoint,3), the bits of xyz at idx.  return_mindist: also mindist (b,n), every point's final
    squared distance to the chosen set (-1 for a non-finite point).
    form: "auto" (by n), "workgroup" (a workgroup per cloud) or "wave" (a wave per cloud, n <= 1024): same bits.
    -> idx, or (idx[, sampled][, mindist])."""
    code = _fps_form(form)
    xyz = _f32(xyz, "xyz", 3)
    if xyz.shape[2] != 3:
        raise ValueError("farthest_point_sample only accepts 3d point sets")
    b, n, _ = xyz.shape
    m = int(npoint)
    if b < 1 or not 1 <= n <= FPS_MAX_POINTS:
        raise ValueError("farthest_point_sample needs b >= 1 clouds of 1 <= n <= %d points (got b=%d, n=%d)" % (FPS_MAX_POINTS, b, n))
    if not 1 <= m <= n:
        raise ValueError("npoint must be in [1, n] (got npoint=%d for n=%d)" % (m, n))
    farthest_point_sample_plan(n, form)                         # ValueError for "wave" beyond its size, before any launch
    dev = xyz.device
    st = _fps_start(start, b, n, dev)
    idx = torch.empty((b, m), dtype=torch.int32, device=dev)
    sampled = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if return_points else None
    mindist = torch.empty((b, n), dtype=torch.float32, device=dev) if return_mindist else None
    with torch.cuda.device(dev):
        _call("geoadv_farthest_point_sample", b, n, _lib.ptr(xyz), m, _lib.ptr(st), code, _lib.ptr(idx), _lib.ptr(sampled), _lib.ptr(mindist))
    out = (idx,) + ((sampled,) if return_points else ()) + ((mindist,) if return_mindist else ())
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------
# the defenses' per-cloud bookkeeping (src/adversary_utils.py:149-178, src/ae_utils.py:12-80), device side
# ---------------------------------------------------------------------------------------------
def outlier_filter(point_clouds, knn_dists, knn_dist_thresh, top_k=None, want_outliers=True):
    """get_outlier_pc_inlier_pc(point_clouds, knn_dists, knn_dist_thresh) (adversary_utils.py:149-178) on GPU tensors ->
    (outlier_pc (b,n,3), outlier_idx (b,n) int16, outlier_num (b,) int16, inlier_pc (b,n,3)).
    knn_dists (b,n): the per-point scalar the reference function thresholds; or (b,n,k) with top_k: the kernel then forms
    the mean of the first top_k distances itself, as run_defense_surface.py:187-191 does with numpy.
    want_outliers=False skips the three outlier outputs (None)."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("outlier_filter only accepts 3d point sets")
    b, n, _ = pc.shape
    if knn_dists.dim() == 2:
        kd, stride, top_k = _f32(knn_dists, "knn_dists", 2), 1, 1
    else:
        kd = _f32(knn_dists, "knn_dists", 3)
        stride = kd.shape[2]
        top_k = stride if top_k is None else int(top_k)
    if tuple(kd.shape[:2]) != (b, n):
        raise ValueError("knn_dists must be of shape (batch, num_points[, k]); got %s for clouds %s" % (tuple(kd.shape), tuple(pc.shape)))
    inlier = torch.empty_like(pc)
    o_pc = torch.empty_like(pc) if want_outliers else None
    o_idx = torch.empty((b, n), dtype=torch.int16, device=pc.device) if want_outliers else None
    o_num = torch.empty((b,), dtype=torch.int16, device=pc.device) if want_outliers else None
    with torch.cuda.device(pc.device):
        _call("geoadv_outlier_filter", b, n, _lib.ptr(pc), _lib.ptr(kd), int(stride), int(top_k), float(knn_dist_thresh),
              _lib.ptr(o_pc), _lib.ptr(o_idx), _lib.ptr(o_num), _lib.ptr(inlier))
    return o_pc, o_idx, o_num, inlier


STAT_DEFENSE_MAX_POINTS = 32767                             # include/geoadv.h geoadv_sor_filter / geoadv_random_drop (int16 indices)
SOR_MAX_KNN = 64
_knn_dists_op = knn_dists                                   # (sor_filter has an argument of that name)


def sor_filter(point_clouds, knn_dists=None, k=2, alpha=1.1, want_outliers=True, return_stats=False):
    """Statistical outlier removal (csrc/stat_defense.hip, the rule in include/geoadv.h): per cloud the float64 mean mu and
    sample variance var of the score s_p = mean(knn_dists[p, :k]), summed in a fixed order; a point is an inlier iff s_p is
    finite and s_p <= mu + alpha * sqrt(var) (tested as (s_p - mu)^2 <= alpha^2 var, without a square root).
    point_clouds (b,n,3), 1 <= n <= 32767.  knn_dists: None (ops.knn_dists(point_clouds, k) is computed here), (b,n,stride)
    with 1 <= k <= stride <= 64, or (b,n), a per-point score of the caller's (k is then 1); squared distances give
    IF-Defense's variant.  alpha >= 0.
    -> (outlier_pc (b,n,3), outlier_idx (b,n) int16, outlier_num (b,) int16, inlier_pc (b,n,3)[, stats (b,3) float64 = mu, var,
    the number of finite scores]), packed and padded as outlier_filter's.  want_outliers=False skips the three outlier
    outputs (None)."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("sor_filter only accepts 3d point sets")
    b, n, _ = pc.shape
    if not 1 <= n <= STAT_DEFENSE_MAX_POINTS:
        raise ValueError("sor_filter needs clouds of 1 <= n <= %d points (got n=%d)" % (STAT_DEFENSE_MAX_POINTS, n))
    alpha = float(alpha)
    if not (alpha >= 0.0 and alpha != float("inf")):
        raise ValueError("alpha must be finite and >= 0 (got %r)" % alpha)
    k = int(k)
    if knn_dists is None:
        if not 1 <= k <= min(SOR_MAX_KNN, n - 1):
            raise ValueError("k must be in [1, min(%d, n - 1)] (got k=%d for n=%d)" % (SOR_MAX_KNN, k, n))
        kd, stride = _knn_dists_op(pc, k), k
    elif isinstance(knn_dists, torch.Tensor) and knn_dists.dim() == 2:
        kd, stride, k = _f32(knn_dists, "knn_dists", 2), 1, 1
    else:
        kd = _f32(knn_dists, "knn_dists", 3)
        stride = kd.shape[2]
    if tuple(kd.shape[:2]) != (b, n):
        raise ValueError("knn_dists must be of shape (batch, num_points[, k]); got %s for clouds %s" % (tuple(kd.shape), tuple(pc.shape)))
    if not 1 <= k <= stride <= SOR_MAX_KNN:
        raise ValueError("sor_filter needs 1 <= k <= knn_dists.shape[2] <= %d (got k=%d, %d columns)" % (SOR_MAX_KNN, k, stride))
    inlier = torch.empty_like(pc)
    o_pc = torch.empty_like(pc) if want_outliers else None
    o_idx = torch.empty((b, n), dtype=torch.int16, device=pc.device) if want_outliers else None
    o_num = torch.empty((b,), dtype=torch.int16, device=pc.device) if want_outliers else None
    stats = torch.empty((b, 3), dtype=torch.float64, device=pc.device) if return_stats else None
    with torch.cuda.device(pc.device):
        _call("geoadv_sor_filter", b, n, _lib.ptr(pc), _lib.ptr(kd), int(stride), k, alpha,
              _lib.ptr(o_pc), _lib.ptr(o_idx), _lib.ptr(o_num), _lib.ptr(inlier), _lib.ptr(stats))
    return (o_pc, o_idx, o_num, inlier) + ((stats,) if return_stats else ())


KNN_LOSS_MAX_K = 15                                         # include/geoadv.h geoadv_knn_outlier_loss
KNN_LOSS_MAX_POINTS = 16384                                 # (the rule's 32767, less what the search takes)


KNN_LOSS_SURFACE_MAX_K = 7                                  # the surface rule: outlier_filter's top_k limit
KNN_LOSS_RULES = {"sor": 0, "surface": _abi.GEOADV_KNN_LOSS_SURFACE}     # OR-ed into the call's kernel argument


def knn_outlier_loss(point_clouds, k=5, alpha=1.05, want_grad=True, return_parts=False, kernel=None, rule="sor", thresh=0.04):
    """The kNN outlier loss of the kNN attack and its gradient (csrc/knn_loss.hip, the rule in include/geoadv.h): per cloud the
    score s_p = the mean SQUARED distance of point p to its k nearest neighbours, SOR's float64 statistics mu and var of it, the
    mask w_p = s_p > mu + alpha * sqrt(var) (tested without a square root: the complement of sor_filter's inliers), the loss
    K = sum(w_p s_p) / n and dK / dx with the mask held constant -- the gather over a masked point's own neighbours plus the
    scatter from the masked points that list it, summed in float64 in a fixed order (no float atomics: repeatable bits).
    point_clouds (b,n,3) float32, 1 <= k <= 15, k + 2 <= n <= 16384, alpha >= 0.  kernel: the k-NN kernel, as knn_point.
    -> (loss (b,) float64, grad (b,n,3) float32 or None without want_grad)[, score (b,n) float64, mask (b,n) bool,
    idx (b,n,k) int32, stats (b,4) float64 = mu, var, the number of finite scores, the number of masked points].
    rule="surface" (GEOADV_KNN_LOSS_SURFACE): the rule of the paper's off-surface defense instead -- s_p the fp32 mean DISTANCE to
    the k <= 7 nearest neighbours, w_p = s_p > float32(thresh), exactly the points outlier_filter(x, knn_dists(x, k), thresh,
    top_k=k) removes, K = sum(w_p (s_p - thresh)) / n and its gradient (unit vectors along the masked points' edges; a zero-length
    edge adds nothing); alpha is then not looked at, score is float64(s_p) and stats = thresh, 0, the number of scores that are
    not NaN, the number of masked points."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("knn_outlier_loss only accepts 3d point sets")
    b, n, _ = pc.shape
    k = int(k)
    if not 1 <= k <= KNN_LOSS_MAX_K:
        raise ValueError("k must be in [1, %d] (got k=%d)" % (KNN_LOSS_MAX_K, k))
    if not k + 2 <= n <= KNN_LOSS_MAX_POINTS:
        raise ValueError("knn_outlier_loss needs clouds of k + 2 = %d <= n <= %d points (got n=%d)" % (k + 2, KNN_LOSS_MAX_POINTS, n))
    if rule not in KNN_LOSS_RULES:
        raise ValueError("rule must be one of %s (got %r)" % (sorted(KNN_LOSS_RULES), rule))
    if rule == "surface":
        if k > KNN_LOSS_SURFACE_MAX_K:
            raise ValueError("rule='surface' takes k in [1, %d], as outlier_filter's top_k (got k=%d)" % (KNN_LOSS_SURFACE_MAX_K, k))
        alpha = float(thresh)                               # the call's alpha is the threshold under the flag
        if not 0.0 <= alpha <= 3.4028234663852886e38:
            raise ValueError("thresh must be finite, >= 0 and within float32 (got %r)" % alpha)
    else:
        alpha = float(alpha)
        if not (alpha >= 0.0 and alpha != float("inf")):
            raise ValueError("alpha must be finite and >= 0 (got %r)" % alpha)
    dev = pc.device
    loss = torch.empty((b,), dtype=torch.float64, device=dev)
    grad = torch.empty_like(pc) if want_grad else None
    score = torch.empty((b, n), dtype=torch.float64, device=dev) if return_parts else None
    mask = torch.empty((b, n), dtype=torch.uint8, device=dev) if return_parts else None
    idx = torch.empty((b, n, k), dtype=torch.int32, device=dev) if return_parts else None
    stats = torch.empty((b, 4), dtype=torch.float64, device=dev) if return_parts else None
    with torch.cuda.device(dev):
        wb = int(_lib.lib().geoadv_knn_outlier_loss_workspace_bytes(b, n, k))
        ws = torch.empty(wb, dtype=torch.uint8, device=dev)
        _call("geoadv_knn_outlier_loss", _knn_kernel(kernel) | KNN_LOSS_RULES[rule], b, n, k, alpha, _lib.ptr(pc), _lib.ptr(loss), _lib.ptr(grad),
              _lib.ptr(score), _lib.ptr(mask), _lib.ptr(idx), _lib.ptr(stats), _lib.ptr(ws), wb)
    return (loss, grad) + ((score, mask.to(torch.bool), idx, stats) if return_parts else ())


def random_drop(point_clouds, drop, seed, counter=0, slot_offset=0, return_idx=False):
    """Simple random sampling (csrc/stat_defense.hip, the rule in include/geoadv.h): every cloud of point_clouds (b,n,3) loses
    the `drop` points with the smallest counter-based 64-bit draws r(seed, counter, slot_offset + cloud, point) -> kept (b,n,3):
    the other points in point order, padded with the last of them[, dropped_idx (b,drop) int32, ascending].
    0 <= drop < n <= 32767; drop == 0 copies the bits.  The result depends on (seed, counter, slot, point) alone, not on the
    batch, torch's generator or the data: ranks that pass slot_offset = rank * local batch draw what one rank would."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("random_drop only accepts 3d point sets")
    b, n, _ = pc.shape
    drop, seed, counter, slot_offset = int(drop), int(seed), int(counter), int(slot_offset)
    if not 1 <= n <= STAT_DEFENSE_MAX_POINTS:
        raise ValueError("random_drop needs clouds of 1 <= n <= %d points (got n=%d)" % (STAT_DEFENSE_MAX_POINTS, n))
    if not 0 <= drop < n:
        raise ValueError("drop must be in [0, n) (got drop=%d for n=%d)" % (drop, n))
    for name, v in (("seed", seed), ("counter", counter)):
        if not 0 <= v < 1 << 64:
            raise ValueError("%s must be in [0, 2^64) (got %d)" % (name, v))
    if not 0 <= slot_offset <= (1 << 32) - b:
        raise ValueError("slot_offset must be >= 0 with slot_offset + batch <= 2^32 (got %d)" % slot_offset)
    kept = torch.empty_like(pc)
    idx = torch.empty((b, drop), dtype=torch.int32, device=pc.device) if return_idx else None
    with torch.cuda.device(pc.device):
        _call("geoadv_random_drop", b, n, _lib.ptr(pc), drop, seed, counter, slot_offset,
              _lib.ptr(kept), _lib.ptr(idx))
    return (kept, idx) if return_idx else kept


def critical_split(point_clouds, max_val, max_idx):
    """get_critical_pc_non_critical_pc (ae_utils.py:51-80) from (np.max, np.argmax)(pre_symmetry, axis=1) on GPU tensors ->
    (critical_points (b,c,3), critical_idx (b,c) int16, critical_num (b,) int16, critical_pc (b,n,3), non_critical_pc (b,n,3)).
    Critical points owning equally many channels come in descending point index (include/geoadv.h)."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("critical_split only accepts 3d point sets")
    b, n, _ = pc.shape
    mv = _f32(max_val, "max_val", 2)
    c = mv.shape[1]
    if mv.shape[0] != b:
        raise ValueError("max_val must be of shape (batch, channels)")
    mi = _i32(max_idx, "max_idx", (b, c))
    cp = torch.empty((b, c, 3), dtype=torch.float32, device=pc.device)
    ci = torch.empty((b, c), dtype=torch.int16, device=pc.device)
    cn = torch.empty((b,), dtype=torch.int16, device=pc.device)
    cpc, ncpc = torch.empty_like(pc), torch.empty_like(pc)
    with torch.cuda.device(pc.device):
        _call("geoadv_critical_split", b, n, c, _lib.ptr(pc), _lib.ptr(mv), _lib.ptr(mi), _lib.ptr(cp), _lib.ptr(ci), _lib.ptr(cn),
              _lib.ptr(cpc), _lib.ptr(ncpc))
    return cp, ci, cn, cpc, ncpc


# ---------------------------------------------------------------------------------------------
# the dataset stage (src/shift_rotate_util.py:22-62), device side
# ---------------------------------------------------------------------------------------------
def sort_axes(point_clouds, neg_rot=True):
    """sort_axes(point_clouds, neg_rot) (shift_rotate_util.py:22-44) on a GPU tensor (b,n,3) -> (sorted clouds (b,n,3),
    axes_idx (b,3) int32 = get_sort_axes_idx's indices).  The longer of the x and y extents becomes x, z stays; equal
    extents are swapped as the reference swaps them ([1,0,2]); axis int(neg_rot) is negated only where x was strictly shorter.
    Bit-equal to the reference (copies and sign flips).  1 <= n <= 16384 (include/geoadv.h)."""
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("sort_axes only accepts 3d point sets")
    b, n, _ = pc.shape
    out = torch.empty_like(pc)
    axes_idx = torch.empty((b, 3), dtype=torch.int32, device=pc.device)
    with torch.cuda.device(pc.device):
        _call("geoadv_sort_axes", b, n, _lib.ptr(pc), _lib.ptr(out), _lib.ptr(axes_idx), int(bool(neg_rot)))
    return out, axes_idx


def _gather_index(index, num_clouds, dev):
    """The source-cloud index of batch_gather / augment_batch -> (b, int32 device tensor or None for 0..num_clouds-1).  A host
    index is range-checked here; a device index is not (the kernels never dereference a bad entry)."""
    import numpy as np
    if index is None:
        return num_clouds, None
    elif isinstance(index, torch.Tensor) and index.is_cuda:
        if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64):
            raise ValueError("index must be a one-dimensional int32 or int64 tensor (got %s of shape %s)" % (index.dtype, tuple(index.shape)))
        idx = index.to(device=dev, dtype=torch.int32).contiguous()
        b = int(idx.numel())
    else:
        host = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
        if host.ndim != 1 or host.dtype.kind not in "iu":
            raise ValueError("index must be a one-dimensional integer array")
        if host.size and (int(host.min()) < 0 or int(host.max()) >= num_clouds):
            raise ValueError("index out of range: values %d .. %d for %d clouds" % (int(host.min()), int(host.max()), num_clouds))
        b = int(host.size)
        idx = torch.from_numpy(host.astype(np.int32)).to(dev)
    return b, idx


def batch_gather(data, index=None, augment=None, rot=None, want_clean=False):
    """One training batch out of resident clouds in one launch (csrc/dataset.hip, geoadv_batch_gather).
    data: GPU float32 (num_clouds, n, 3).  index: the source cloud of every output cloud -- a host sequence / numpy array
    (range-checked here: ValueError before any launch) or a device integer tensor (not checked on the host: the kernel never
    reads outside data and leaves the slot of a bad index unwritten); None = every cloud of data in order.
    augment: None, a BatchAugment or a dict of its fields (seed, counter, slot_offset, noise_mu, noise_sigma, noise_clip,
    rotate_first).  rot: None, or rotation matrices (3, 3) for the whole batch / (b, 3, 3) one per cloud, numpy or a float64
    GPU tensor; a point is a row vector times its matrix, in float64.
    -> feed (b, n, 3), or (clean, feed) with want_clean: clean holds the bits of data[index]."""
    import numpy as np
    data = _f32(data, "data", 3)
    if data.shape[2] != 3:
        raise ValueError("batch_gather only accepts 3d point sets")
    num_clouds, n, _ = data.shape
    dev = data.device
    b, idx = _gather_index(index, num_clouds, dev)
    if b < 1 or n < 1:
        raise ValueError("batch_gather needs at least one cloud and one point (b=%d, n=%d)" % (b, n))
    aug = None
    if isinstance(augment, BatchAugment):
        aug = BatchAugment.from_buffer_copy(augment)
    elif augment is not None:
        unknown = set(augment) - {f for f, _ in BatchAugment._fields_ if f != "rot_count"}
        if unknown:
            raise ValueError("unknown augment fields %s" % sorted(unknown))
        aug = BatchAugment(**augment)
    rot_dev = None
    if rot is not None:
        if aug is None:
            aug = BatchAugment()
        if isinstance(rot, torch.Tensor):
            rot_dev = rot.to(device=dev, dtype=torch.float64)
        else:
            rot_dev = torch.from_numpy(np.ascontiguousarray(rot, dtype=np.float64)).to(dev)
        if rot_dev.dim() == 2:
            rot_dev = rot_dev[None]
        if rot_dev.dim() != 3 or tuple(rot_dev.shape[1:]) != (3, 3) or rot_dev.shape[0] not in (1, b):
            raise ValueError("rot must be (3, 3) or (%d, 3, 3); got %s" % (b, tuple(rot_dev.shape)))
        rot_dev = rot_dev.contiguous()
        aug.rot_count = int(rot_dev.shape[0])
    elif aug is not None:
        aug.rot_count = 0
    feed = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    clean = torch.empty_like(feed) if want_clean else None
    with torch.cuda.device(dev):
        _call("geoadv_batch_gather", b, n, _lib.ptr(data), num_clouds, _lib.ptr(idx),
              C.byref(aug) if aug is not None else None, _lib.ptr(rot_dev), _lib.ptr(clean), _lib.ptr(feed))
    return (clean, feed) if want_clean else feed


# ---------------------------------------------------------------------------------------------
# AtlasNet's data side (transfer/atlasnet/dataset/pointcloud_processor.py, augmenter.py), device side
# ---------------------------------------------------------------------------------------------
NORMALIZATIONS = {"Identity": _abi.GEOADV_NORMALIZE_IDENTITY, "UnitBall": _abi.GEOADV_NORMALIZE_UNIT_BALL,
                  "BoundingBox": _abi.GEOADV_NORMALIZE_BOUNDING_BOX}


def normalize_clouds(point_clouds, normalization="UnitBall"):
    """Normalization.normalize_unitL2ball_functional / normalize_bounding_box_functional / identity_functional
    (pointcloud_processor.py:160-233) on a GPU tensor (b,n,3) -> a new tensor (b,n,3).  UnitBall: minus the cloud's mean, times
    1 / sqrt(max ||p - mean||^2); BoundingBox: minus (min + max) / 2 per axis, times 1 / max_axis((max - min) / 2).  Centre and
    factor are float64 and bitwise reproducible; (x - c) * s is rounded to fp32 once.  A cloud whose points all coincide, or
    that holds a NaN, comes out all NaN, as in the reference.  1 <= n <= 2^20 (include/geoadv.h)."""
    if normalization not in NORMALIZATIONS:
        raise ValueError("normalization must be one of %s; got %r" % (sorted(NORMALIZATIONS), normalization))
    pc = _f32(point_clouds, "point_clouds", 3)
    if pc.shape[2] != 3:
        raise ValueError("normalize_clouds only accepts 3d point sets")
    b, n, _ = pc.shape
    out = torch.empty_like(pc)
    with torch.cuda.device(pc.device):
        _call("geoadv_normalize_clouds", b, n, NORMALIZATIONS[normalization], _lib.ptr(pc), _lib.ptr(out))
    return out


AUGMENT_RECORD = _abi.GEOADV_AUGMENT_RECORD     # 3 axial matrices, the 3-D matrix, scale, flip, translation


def augment_batch(data, index=None, config=None, params=None, n_out=None, want_params=False):
    """One AtlasNet training batch out of resident clouds in one launch (csrc/dataset.hip, geoadv_augment_batch): gather,
    re-sampling, then the Augmenter's operators in its order (axial rotations, 3-D rotation, scale, flips, translation).
    data: GPU float32 (num_clouds, n_src, 3).  index: as batch_gather's -- a host sequence (range-checked here), a device
    integer tensor (a bad entry leaves its slot unwritten) or None = every cloud in order.
    config: None (plain gather), a CloudAugment or a dict of its fields; fields left out of a dict take the reference's
    defaults (CloudAugment.DEFAULTS), unknown keys are refused.  `sample` is set from n_out when the dict leaves it out.
    n_out: points per output cloud; None = n_src.  Without sample it must equal n_src.
    params: None, or explicit operators (b, 45) float32 (numpy or GPU): the enabled operators are taken from it, nothing is drawn.
    -> out (b, n_out, 3), or (out, params (b, 45)) with want_params: the record that was applied (layout: include/geoadv.h)."""
    import numpy as np
    data = _f32(data, "data", 3)
    if data.shape[2] != 3:
        raise ValueError("augment_batch only accepts 3d point sets")
    num_clouds, n_src, _ = data.shape
    dev = data.device
    b, idx = _gather_index(index, num_clouds, dev)
    n_out = n_src if n_out is None else int(n_out)
    if b < 1 or n_src < 1 or n_out < 1:
        raise ValueError("augment_batch needs at least one cloud and one point (b=%d, n_src=%d, n_out=%d)" % (b, n_src, n_out))
    cfg = None
    if isinstance(config, CloudAugment):
        cfg = CloudAugment.from_buffer_copy(config)
    elif config is not None:
        unknown = set(config) - {f for f, _ in CloudAugment._fields_}
        if unknown:
            raise ValueError("unknown config fields %s" % sorted(unknown))
        fields = dict(CloudAugment.DEFAULTS, **config)
        fields.setdefault("sample", int(n_out != n_src))
        cfg = CloudAugment(**fields)
    par = None
    if params is not None:
        par = params if isinstance(params, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32))
        par = par.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(par.shape) != (b, AUGMENT_RECORD):
            raise ValueError("params must be (%d, %d); got %s" % (b, AUGMENT_RECORD, tuple(par.shape)))
    out = torch.empty((b, n_out, 3), dtype=torch.float32, device=dev)
    par_out = torch.empty((b, AUGMENT_RECORD), dtype=torch.float32, device=dev) if want_params else None
    with torch.cuda.device(dev):
        _call("geoadv_augment_batch", b, n_out, _lib.ptr(data), num_clouds, n_src, _lib.ptr(idx),
              C.byref(cfg) if cfg is not None else None, _lib.ptr(par), _lib.ptr(par_out), _lib.ptr(out))
    return (out, par_out) if want_params else out


# ---------------------------------------------------------------------------------------------
# classifier/provider.py, device side
# ---------------------------------------------------------------------------------------------
def rotate_point_cloud_by_angle(batch_data, rotation_angle):
    """provider.rotate_point_cloud_by_angle on a GPU tensor (b,n,3): every point, as a row vector, times
    [[c,0,s],[0,1,0],[-s,0,c]] with c, s = np.cos / np.sin of rotation_angle (float64, computed here on the host as the
    reference computes them); the float32 coordinates are multiplied and summed in float64 on the device and rounded once, as
    numpy's float32 @ float64 product stored into a float32 array."""
    import numpy as np
    pc = _f32(batch_data, "batch_data", 3)
    if pc.shape[2] != 3:
        raise ValueError("rotate_point_cloud_by_angle only accepts 3d point sets")
    b, n, _ = pc.shape
    out = torch.empty_like(pc)
    with torch.cuda.device(pc.device):
        _call("geoadv_rotate_y", b, n, _lib.ptr(pc), float(np.cos(rotation_angle)),
              float(np.sin(rotation_angle)), _lib.ptr(out))
    return out


# ---------------------------------------------------------------------------------------------
# external/structural_losses/tf_approxmatch.py
# ---------------------------------------------------------------------------------------------
EMD_FAST, EMD_REFERENCE = _abi.GEOADV_EMD_FAST, _abi.GEOADV_EMD_REFERENCE      # how the pair weight expf(level * d2) is evaluated
EMD_DENSE_LEVELS = _abi.GEOADV_EMD_DENSE_LEVELS                          # ... | this flag: every sweep of the call dense (no cell-grid form of the first three levels)


def emd_sparse_levels(on):
    """TESTS / MEASUREMENTS: the process default of EMD calls that pass no `dense_levels` (include/geoadv.h)."""
    _lib.check(_lib.lib().geoadv_emd_sparse_levels(int(bool(on))), "emd_sparse_levels")


def _emd_mode(reference_weights, dense_levels):
    return (EMD_REFERENCE if reference_weights else EMD_FAST) | (EMD_DENSE_LEVELS if dense_levels else 0)


def approx_match(xyz1, xyz2, reference_weights=False, dense_levels=False):
    """tf_approxmatch.py:10-18.  xyz1 (b,n,3), xyz2 (b,m,3) -> match (b,m,n): match[b,l,k] is the
    soft assignment between xyz2 point l and xyz1 point k (the reference GPU op's layout; the CPU
    op writes the transpose into the same declared shape).  Level schedule of the CPU op.
    reference_weights: every pair weight bit for bit the CPU op's (GEOADV_EMD_REFERENCE: every plan entry within ~2 float
    ulps of the CPU op, ~3.7x the time) instead of the fp32 fast form (typically 1e-6, rare entries 1e-4 relative).
    dense_levels: every sweep of THIS call dense (per call; the results differ only in the order of fp64 additions)."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "ApproxMatch")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    match = torch.empty((b, m, n), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        nf = _lib.lib().geoadv_approx_match_temp_floats(b, n, m)
        temp = torch.empty(int(nf), dtype=torch.float32, device=xyz1.device)
        _call("geoadv_approx_match_mode", _emd_mode(reference_weights, dense_levels), b, n, m, _lib.ptr(xyz1), _lib.ptr(xyz2),
              _lib.ptr(match), _lib.ptr(temp))
    return match


def _match_args(xyz1, xyz2, match, op):
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, op)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    match = _f32(match, "match", 3)
    if tuple(match.shape) != (b, m, n):
        raise ValueError("%s expects (batch_size,#query,#dataset) match shape" % op)      # tf_approxmatch.cpp
    return xyz1, xyz2, match, b, n, m


def match_cost(xyz1, xyz2, match):
    """tf_approxmatch.py:21-32 -> cost (b,): sum over pairs of match * euclidean distance."""
    xyz1, xyz2, match, b, n, m = _match_args(xyz1, xyz2, match, "MatchCost")
    cost = torch.empty((b,), dtype=torch.float32, device=xyz1.device)
    with torch.cuda.device(xyz1.device):
        wf = int(_lib.lib().geoadv_match_cost_workspace_floats(b, n, m))
        ws = torch.empty(wf, dtype=torch.float32, device=xyz1.device)
        _call("geoadv_match_cost_ws", b, n, m, _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(match), _lib.ptr(cost), _lib.ptr(ws), wf)
    return cost


def match_cost_grad(xyz1, xyz2, match):
    """The MatchCostGrad op behind tf_approxmatch.py:38-50 -> (grad1 (b,n,3), grad2 (b,m,3)),
    before the scaling by the upstream grad_cost[b]."""
    xyz1, xyz2, match, b, n, m = _match_args(xyz1, xyz2, match, "MatchCostGrad")
    g1 = torch.empty_like(xyz1)
    g2 = torch.empty_like(xyz2)
    with torch.cuda.device(xyz1.device):
        _call("geoadv_match_cost_grad", b, n, m, _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(match), _lib.ptr(g1), _lib.ptr(g2))
    return g1, g2


def emd_cost_grad1(xyz1, xyz2, reference_weights=False, dense_levels=False):
    """match_cost(xyz1, xyz2, approx_match(xyz1, xyz2)) and its gradient w.r.t. xyz1 with the plan held constant, without
    materialising the (b,m,n) plan -- the fused form the attack loop uses.  -> (cost (b,), grad1 (b,n,3))."""
    xyz1, xyz2 = _xyz_pair(xyz1, xyz2, "ApproxMatch")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    cost = torch.empty((b,), dtype=torch.float32, device=xyz1.device)
    g1 = torch.empty_like(xyz1)
    with torch.cuda.device(xyz1.device):
        nf = _lib.lib().geoadv_emd_cost_grad1_temp_floats(b, n, m)
        temp = torch.empty(int(nf), dtype=torch.float32, device=xyz1.device)
        _call("geoadv_emd_cost_grad1_mode", _emd_mode(reference_weights, dense_levels), b, n, m, _lib.ptr(xyz1), _lib.ptr(xyz2),
              _lib.ptr(cost), _lib.ptr(g1), _lib.ptr(temp))
    return cost, g1


class _MatchCostFn(torch.autograd.Function):
    """@tf.RegisterGradient('MatchCost') (tf_approxmatch.py:38-50): grads scaled by grad_cost[b],
    no gradient w.r.t. match (ApproxMatch is registered NoGradient, :19)."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, match):
        ctx.save_for_backward(xyz1, xyz2, match)
        return match_cost(xyz1, xyz2, match)

    @staticmethod
    def backward(ctx, grad_cost):
        xyz1, xyz2, match = ctx.saved_tensors
        g1, g2 = match_cost_grad(xyz1, xyz2, match)
        gc = grad_cost.reshape(-1, 1, 1)
        return g1 * gc, g2 * gc, None


def match_cost_autograd(xyz1, xyz2, match):
    return _MatchCostFn.apply(xyz1, xyz2, match)


# ---------------------------------------------------------------------------------------------
# attacker/prepare_indices_for_attack.py
# ---------------------------------------------------------------------------------------------
def chamfer_dist_matrix(pcs_a, pcs_b, max_workspace_bytes=2 << 30):
    """All-pairs Chamfer distance: out[i, j] = mean(dist1) + mean(dist2) of nn_distance(pcs_a[i], pcs_b[j])
    (the `chamfer_dist` tensor of prepare_indices_for_attack.py:113-114 for every pair), computed without
    tiling the clouds.  pcs_a (na,n,3), pcs_b (nb,m,3) GPU tensors -> (na, nb)."""
    a = _f32(pcs_a, "pcs_a", 3)
    b = _f32(pcs_b, "pcs_b", 3)
    if a.shape[2] != 3 or b.shape[2] != 3:
        raise ValueError("chamfer_dist_matrix only accepts 3d point sets")
    na, n, _ = a.shape
    nb, m, _ = b.shape
    out = torch.empty((na, nb), dtype=torch.float32, device=a.device)
    if na == 0 or nb == 0:
        return out
    with torch.cuda.device(a.device):
        want = _lib.lib().geoadv_chamfer_matrix_workspace_floats(na, nb, n, m)
        nfl = int(min(want, max(max_workspace_bytes // 4, _lib.lib().geoadv_chamfer_matrix_workspace_floats(1, 1, n, m))))
        ws = torch.empty(nfl, dtype=torch.float32, device=a.device)
        st = _lib.lib().geoadv_chamfer_matrix(na, nb, n, m, _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), _lib.ptr(ws),
                                              nfl, _lib.stream_handle())
    _lib.check(st, "chamfer_matrix")
    return out


LATENT_DIST_MAX_D = 128         # include/geoadv.h geoadv_latent_dist_matrix


def latent_dist_matrix(a, b=None):
    """All-pairs Euclidean distance of latent codes: out[i, j] = ||a[i] - b[j]||_2, the matrix of get_dist_mat
    (src/general_utils.py:94-106) behind prepare_indices_for_attack.py:89-101, without its tiled (n, n, d) copies.
    a (na,d), b (nb,d) float32 GPU tensors (b=None: b = a) -> (na, nb).  The bits of np.linalg.norm(s - t, axis=-1) (numpy's
    summation order; csrc/latent_dist.hip); for b = a exactly symmetric with a +0 diagonal.  1 <= d <= 128."""
    a = _f32(a, "a", 2)
    b = a if b is None else _f32(b, "b", 2)
    if b.device != a.device:
        raise ValueError("a and b must live on the same device (got %s and %s)" % (a.device, b.device))
    if a.shape[1] != b.shape[1]:
        raise ValueError("latent_dist_matrix expects a and b of the same width (got %d and %d)" % (a.shape[1], b.shape[1]))
    d = a.shape[1]
    if not 1 <= d <= LATENT_DIST_MAX_D:
        raise ValueError("latent_dist_matrix supports 1 <= d <= %d (got %d)" % (LATENT_DIST_MAX_D, d))
    na, nb = a.shape[0], b.shape[0]
    out = torch.empty((na, nb), dtype=torch.float32, device=a.device)
    if na == 0 or nb == 0:
        return out
    with torch.cuda.device(a.device):
        _call("geoadv_latent_dist_matrix", na, nb, d, _lib.ptr(a), _lib.ptr(b), _lib.ptr(out))
    return out


# ---------------------------------------------------------------------------------------------
# the training steps' GEMM kernels on their own (tests and tools)
# ---------------------------------------------------------------------------------------------
TRAIN_GEMM_SPLITK, TRAIN_GEMM_TILE = 0, 1       # include/geoadv.h geoadv_train_gemm's `kernel`


def train_gemm(kernel, a, a_strides, b, b_strides, c, c_strides, bias, bias_stride, m, n, k, batch=1):
    """geoadv_train_gemm: c[z][i * ldc + j] = sum_k a[z * sAz + i * sAi + k * sAk] * b[z * sBz + k * sBk + j * sBj] + bias[z * sBiasZ + j]
    on float32 GPU tensors that are read and written from their first element on with the strides given (in floats): a_strides =
    (sAi, sAk, sAz), b_strides = (sBk, sBj, sBz), c_strides = (ldc, sCz); bias may be None.  Nothing is reshaped or copied: the
    caller owns the layout.  kernel: TRAIN_GEMM_SPLITK (csrc/train_tile.h) or TRAIN_GEMM_TILE (csrc/atlas_train.hip).
    -> the split of the K range the launch took (1 for TRAIN_GEMM_TILE)."""
    for t, name in ((a, "a"), (b, "b"), (c, "c")) + (((bias, "bias"),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError("%s must be a float32 GPU tensor" % name)
    ks = C.c_int(0)
    with torch.cuda.device(c.device):
        part, nf = None, 0
        if kernel == TRAIN_GEMM_SPLITK:
            nf = int(_lib.lib().geoadv_train_gemm_partial_floats())
            part = torch.empty(nf, dtype=torch.float32, device=c.device)      # caller-owned scratch (torch's caching allocator)
        st = _lib.lib().geoadv_train_gemm(int(kernel), _lib.ptr(a), int(a_strides[0]), int(a_strides[1]), int(a_strides[2]), _lib.ptr(b),
                                          int(b_strides[0]), int(b_strides[1]), int(b_strides[2]), _lib.ptr(c), int(c_strides[0]),
                                          int(c_strides[1]), _lib.ptr(bias), int(bias_stride), int(m), int(n), int(k), int(batch),
                                          _lib.ptr(part), nf, C.byref(ks), _lib.stream_handle())
    _lib.check(st, "train_gemm")
    return ks.value


# ---------------------------------------------------------------------------------------------
# the FoldingNet training step's pool and global-maximum kernels on their own (tests and tools)
# ---------------------------------------------------------------------------------------------
def _train_buffers(*named):
    for t, name, dtype in named:
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
            raise ValueError("%s must be a %s GPU tensor" % (name, str(dtype).replace("torch.", "")))


def fold_train_pool(b, n, c, h, cols, g, win):
    """geoadv_fold_train_pool: the training step's graph pool (csrc/fold_train.hip) through the step's own launch.  h float32
    [b n][c], cols int32 [b n][16] rows of the point's cloud in [0, n) -> g float32 [b n][c], win int32 [b n][c] (written).  The
    tensors are read and written from their first element on: nothing is reshaped or copied, the caller owns the layout."""
    _train_buffers((h, "h", torch.float32), (cols, "cols", torch.int32), (g, "g", torch.float32), (win, "win", torch.int32))
    with torch.cuda.device(h.device):
        _call("geoadv_fold_train_pool", int(b), int(n), int(c), _lib.ptr(h), _lib.ptr(cols), _lib.ptr(g), _lib.ptr(win))


def fold_train_pool_grad(b, n, c, dg, win, off, deg, col, dh):
    """geoadv_fold_train_pool_grad: the pool's backward through the step's own launch.  dg float32 and win int32 [b n][c]; off, deg
    int32 [b n] and col int32 [b][32 n], the adjacency rows in the layout of csrc/fold_graph.h -> dh float32 [b n][c] (written)."""
    _train_buffers((dg, "dg", torch.float32), (win, "win", torch.int32), (off, "off", torch.int32), (deg, "deg", torch.int32),
                   (col, "col", torch.int32), (dh, "dh", torch.float32))
    with torch.cuda.device(dg.device):
        _call("geoadv_fold_train_pool_grad", int(b), int(n), int(c), _lib.ptr(dg), _lib.ptr(win), _lib.ptr(off), _lib.ptr(deg),
              _lib.ptr(col), _lib.ptr(dh))


def fold_train_gmax(b, n, c, a, inv, shift, pooled, arg):
    """geoadv_fold_train_gmax: the global maximum of the FoldingNet training step (csrc/train_bn.h, fold_train.hip's copy) through
    the step's own launch.  a float32 [b n][c]; inv, shift float32 [c] -> pooled float32 [b][c], arg int32 [b][c] (written)."""
    _train_buffers((a, "a", torch.float32), (inv, "inv", torch.float32), (shift, "shift", torch.float32),
                   (pooled, "pooled", torch.float32), (arg, "arg", torch.int32))
    with torch.cuda.device(a.device):
        _call("geoadv_fold_train_gmax", int(b), int(n), int(c), _lib.ptr(a), _lib.ptr(inv), _lib.ptr(shift), _lib.ptr(pooled),
              _lib.ptr(arg))
