"""TEST INFRASTRUCTURE: cases, fp64 references and checks of the evaluation kernels (csrc/eval_metrics.hip through maed_amd/eval_utils.py), shared by the
host-simulator tests (tests/test_hostsim_eval_edges.py) and the GPU tests (tests/test_gpu_eval.py).

The references are fp64 torch statements of the four operations written from their definitions (reference: lib/utils/eval_utils.py, lib/core/evaluate.py:139-164),
on the fp32-rounded inputs the kernel sees.  Inputs come from seeded generators; a reference is computed once per case and never modified.

Where the covariance K = X1^T X2 has rank <= 1 the optimal rotation is free about an axis, so the aligned set itself is not determined.  What is determined there
-- the optimal residual var2 - (s1 + s2 + d s3)^2 / var1, the mean of the aligned set, and that the output is a proper similarity image of S1 -- is what those
cases compare (check_similarity)."""
import functools

import torch

from maed_amd import _lib as L
from maed_amd import eval_utils as EU
from maed_amd import ops

# ---- bars ----------------------------------------------------------------------------------------------------------------------------
SCALAR = dict(rtol=1e-5, atol=1e-6)     # MPJPE, PA-MPJPE (where unique), acceleration, vertex error: the bar of tests/test_hostsim_eval.py, here against fp64
# aligned points where unique, max|got - ref| / max|ref| per case.  The kernel aligns in fp64 and rounds once to fp32: the floor is half an fp32 ulp of the
# largest coordinate, 2^-24 = 5.96e-8.  Measured maximum over the unique cases: 5.910e-8 on the host simulator, 5.910e-8 on the MI355X; the bound is 8 x the
# larger (the margin for the summation order of the 64-lane tree), far below the cap of 1e-5.
ALIGNED_REL = 8 * 5.910e-8
# |sum of squared residuals - closed-form optimum| <= 1e-5 * var2.  Measured maximum: 8.05e-8 on the host simulator, 7.34e-8 on the MI355X (the fp32 rounding of
# the aligned points); a rank-1 projection in place of a rotation misses it by 2 % of var2 and more.
RESIDUAL_REL = 1e-5
UNIQUE_GAP = 1e-6                       # the aligned set is compared where s2 + d s3 > 1e-6 s1
MEASURED = {"aligned": 0.0, "residual": 0.0}      # running maxima of the two figures above over the cases a process has run (printed by the test files)

GUARD = 256          # bytes on either side of a guarded output
SENTINEL = 0xA5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(*shape, seed):
    return torch.randn(*shape, generator=_gen(seed))


def _rotation(N, seed):
    """(N,3,3) fp64 proper rotations"""
    Q, _ = torch.linalg.qr(_randn(N, 3, 3, seed=seed).double())
    return Q * torch.sign(torch.linalg.det(Q))[:, None, None]


def _dyadic(*shape, seed):
    """N(0,1) rounded to multiples of 2^-10: products with the few-bit constants below are exact in fp32"""
    return torch.round(_randn(*shape, seed=seed) * 1024) / 1024


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------------
def similarity_ref(S1, S2):
    """orthogonal Procrustes with scale of (N,J,3) sets: S1_hat = s R S1 + t closest to S2, det R = +1 (eval_utils.py:201-252 in fp64)"""
    S1, S2 = S1.float().double(), S2.float().double()
    mu1, mu2 = S1.mean(1, keepdim=True), S2.mean(1, keepdim=True)
    X1, X2 = S1 - mu1, S2 - mu2
    var1, var2 = X1.pow(2).sum((1, 2)), X2.pow(2).sum((1, 2))
    K = X1.transpose(1, 2) @ X2                                               # (N,3,3), K[i][j] = sum_n X1[n][i] X2[n][j]
    U, sig, Vh = torch.linalg.svd(K)
    d = torch.sign(torch.linalg.det(U @ Vh))                                  # det(U V^T)
    Z = torch.eye(3, dtype=torch.float64).repeat(len(S1), 1, 1)
    Z[:, 2, 2] = d
    R = Vh.transpose(1, 2) @ Z @ U.transpose(1, 2)
    s = (R @ K).diagonal(dim1=1, dim2=2).sum(1) / var1
    t = mu2.transpose(1, 2) - s[:, None, None] * (R @ mu1.transpose(1, 2))    # (N,3,1)
    hat = (s[:, None, None] * (R @ S1.transpose(1, 2)) + t).transpose(1, 2)
    opt = var2 - (sig[:, 0] + sig[:, 1] + d * sig[:, 2]).pow(2) / var1       # needs no R: unique even where R is not
    sx = torch.linalg.svdvals(X1)
    return dict(hat=hat, opt=opt, var1=var1, var2=var2, mu2=mu2[:, 0], sig=sig, d=d, unique=sig[:, 1] + d * sig[:, 2] > UNIQUE_GAP * sig[:, 0],
                s1_rank3=sx[:, -1] > 1e-6 * sx[:, 0] if S1.shape[1] >= 3 else torch.zeros(len(S1), dtype=torch.bool), X1=X1, S2=S2)


def pose_ref(pred, target):
    """evaluate.py:139-160: (N,J,3) predictions, (N,J,4) targets [x,y,z,vis] -> dict(mpjpe, pa, pred_c, target_c, sim)"""
    pred, target = pred.float().double(), target.float().double()
    vis = target[..., 3:]
    p, g = pred * vis, target[..., :3] * vis
    p = p - (p[:, 2:3] + p[:, 3:4]) / 2.0
    g = g - (g[:, 2:3] + g[:, 3:4]) / 2.0
    mpjpe = (p - g).pow(2).sum(-1).sqrt().mean(-1)
    sim = similarity_ref(p, g)
    pa = (sim["hat"] - g).pow(2).sum(-1).sqrt().mean(-1)
    return dict(mpjpe=mpjpe, pa=pa, pred_c=p, target_c=g, sim=sim)


def accel_ref(joints, joints_gt=None, vis=None):
    """eval_utils.py:10-21 / :24-52: mean joint norm of the second difference (of the difference to the ground truth); `vis` drops windows touching an invisible frame"""
    a = joints.float().double()
    a = a[:-2] - 2 * a[1:-1] + a[2:]
    if joints_gt is not None:
        b = joints_gt.float().double()
        a = a - (b[:-2] - 2 * b[1:-1] + b[2:])
    out = a.pow(2).sum(2).sqrt().mean(1)
    if vis is not None:
        invis = ~vis.bool()
        out = out[~(invis | torch.roll(invis, -1) | torch.roll(invis, -2))[:-2]]
    return out


def vertex_ref(pred_verts, target_verts):
    """eval_utils.py:88-90"""
    return (pred_verts.float().double() - target_verts.float().double()).pow(2).sum(2).sqrt().mean(1)


# ---- similarity-transform cases ---------------------------------------------------------------------------------------------------------------------
# (kind, N, J).  N in {1, 4, 5, 9}: one wave, a whole workgroup, a workgroup + 1 frame, two workgroups + 1; 4099 frames for the grid.
# J in {2, 3, 4, 14, 17, 49, 63, 64}: the lanes of the wave that carry a joint, up to all of them.
SIM_CASES = [("generic", N, 14) for N in (1, 4, 5, 9, 4099)] + [("generic", 5, J) for J in (2, 3, 4, 17, 49, 63, 64)] + [("generic", 1, 2), ("generic", 9, 64)] + [
    ("similarity", 5, 14), ("similarity", 4, 3), ("similarity", 9, 64),
    ("mirrored", 5, 14), ("mirrored", 4, 4),
    ("inversion", 5, 14), ("inversion", 1, 64),
    ("planar_s1", 5, 14), ("planar_s2", 5, 14), ("planar_both", 5, 14), ("planar_s1", 4, 17), ("planar_s2", 9, 4), ("planar_both", 1, 63),
    ("axis_s1", 5, 14), ("axis_s1", 9, 4),
    ("axis_s2", 5, 14), ("axis_s2", 4, 4), ("axis_s2", 9, 64), ("axis_s2", 1, 17),      # rank-1 K with K v2 exactly zero
    ("line_s2", 5, 14), ("line_s2", 4, 63), ("line_s2", 9, 3),
    ("nearline_s2", 5, 14),
    ("const_s2", 5, 14), ("const_s2", 4, 2),
    ("const_s1", 5, 14), ("generic", 5, 1),                                                # var1 = 0: NaN on both sides
    ("scale_1e-3", 5, 14), ("scale_1e+3", 5, 14), ("scale_1e-3", 4, 49), ("scale_1e+3", 9, 17),
    ("layout_3J", 5, 14), ("layout_3J", 9, 17),
    ("fp64", 5, 14), ("noncontiguous", 5, 14),
]


@functools.lru_cache(maxsize=None)
def sim_inputs(kind, N, J):
    """(S1, S2) as the caller passes them -- CPU tensors; (N,J,3) except for layout_3J"""
    seed = 1000 * len(kind) + 17 * N + J
    S1, S2 = _randn(N, J, 3, seed=seed), _randn(N, J, 3, seed=seed + 1)
    ax = torch.arange(N) % 3                                                 # frame n uses coordinate n % 3
    keep = torch.nn.functional.one_hot(ax, 3)[:, None, :].float()            # (N,1,3): 1 on that coordinate
    if kind in ("similarity", "mirrored"):
        s = torch.rand(N, generator=_gen(seed + 2)).double() + 0.5
        X = S1.double() * (torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64) if kind == "mirrored" else 1.0)
        S2 = (s[:, None, None] * (X @ _rotation(N, seed + 3).transpose(1, 2)) + _randn(N, 1, 3, seed=seed + 4).double()).float()
    elif kind == "inversion":
        S2 = -S1
    elif kind == "planar_s1":
        S1 = S1 * (1 - keep)
    elif kind == "planar_s2":
        S2 = S2 * (1 - keep)
    elif kind == "planar_both":
        S1, S2 = S1 * (1 - keep), S2 * (1 - keep.roll(1, 0) if N > 1 else 1 - keep)
    elif kind == "axis_s1":
        S1 = S1 * keep
    elif kind == "axis_s2":
        S2 = S2 * keep
    elif kind in ("line_s2", "nearline_s2"):
        S2 = _dyadic(N, J, 1, seed=seed + 5) * torch.tensor([0.75, -0.5, 1.25]) + torch.tensor([0.5, -1.0, 2.0])       # exactly collinear in fp32
        if kind == "nearline_s2":
            S2 = S2 + 1e-6 * _randn(N, J, 3, seed=seed + 6)
    elif kind == "const_s2":
        S2 = S2[:, :1].expand(N, J, 3).contiguous()
    elif kind == "const_s1":
        S1 = S1[:, :1].expand(N, J, 3).contiguous()
    elif kind.startswith("scale_"):
        S1, S2 = S1 * float(kind[6:]), S2 * float(kind[6:])
    elif kind == "layout_3J":
        S1, S2 = S1.permute(0, 2, 1).contiguous(), S2.permute(0, 2, 1).contiguous()
    elif kind == "fp64":
        S1, S2 = _randn(N, J, 3, seed=seed).double() + 1e-9, S2.double() - 1e-9                                    # not representable in fp32
    elif kind == "noncontiguous":
        S1, S2 = _randn(N, 2 * J, 3, seed=seed)[:, ::2], _randn(N, J, 5, seed=seed + 1)[:, :, 1:4]
        assert not S1.is_contiguous() and not S2.is_contiguous()
    else:
        assert kind == "generic", kind
    return S1, S2


def _njs(kind, S):
    return S.permute(0, 2, 1) if kind == "layout_3J" else S


@functools.lru_cache(maxsize=None)
def sim_reference(kind, N, J):
    S1, S2 = sim_inputs(kind, N, J)
    return similarity_ref(_njs(kind, S1), _njs(kind, S2))


def close(name, got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| elementwise, no NaN; prints the measured maximum (the host-simulator tests' counterpart of tests/_util.report)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert not bool(torch.isnan(got).any()), name
    err = (got - ref).abs()
    print(f"{name:58s} max_abs={float(err.max()):.3e} ref_max={float(ref.abs().max()):.3e}")
    bad = err > atol + rtol * ref.abs()
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} elements out of tolerance, max_abs={float(err.max()):.3e}"


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check_similarity(hat, ref, tag, note=print, nan_frames=None):
    """`hat` (N,J,3) fp32 kernel output against similarity_ref's dict.  Frames with var1 = 0 are NaN on both sides; frames with a unique optimum compare the
    aligned points; every finite frame compares the residual with the closed-form optimum; rank <= 1 frames compare what is determined."""
    hat = hat.detach().cpu().double()
    assert hat.shape == ref["hat"].shape, (tag, hat.shape)
    nan = torch.isnan(ref["hat"]).any(2).any(1)
    assert bool((ref["var1"][nan] == 0).all()), tag
    if nan_frames is not None:
        assert nan.tolist() == nan_frames, (tag, nan.tolist())
    assert bool(torch.isnan(hat[nan]).all()), f"{tag}: var1 = 0 must give NaN as in the reference"
    assert not bool(torch.isnan(hat[~nan]).any()), f"{tag}: NaN in a frame whose reference is finite"
    uni, free = ref["unique"] & ~nan, ~ref["unique"] & ~nan
    if "nearline" in tag:               # s2 ~ 1e-6 s1, on the edge of the uniqueness criterion: the residual only
        uni, free = uni & False, free & False
    if bool(uni.any()):
        rel = max(_rel(hat[n], ref["hat"][n]) for n in torch.nonzero(uni).flatten().tolist())
        MEASURED["aligned"] = max(MEASURED["aligned"], rel)
        note(f"{tag:58s} aligned points: max|got-ref|/max|ref| = {rel:.3e} over {int(uni.sum())} unique frames (bound {ALIGNED_REL:.2e})")
        assert rel <= ALIGNED_REL, f"{tag}: aligned points differ from the fp64 reference by {rel:.3e} of the largest coordinate (> {ALIGNED_REL:.2e})"
    ok = ~nan
    if bool(ok.any()):
        res = (hat - ref["S2"]).pow(2).sum((1, 2))
        gap = ((res - ref["opt"]).abs() / ref["var2"].clamp_min(1e-300))[ok & (ref["var2"] > 0)]
        exact = (res - ref["opt"]).abs()[ok & (ref["var2"] == 0)]             # S2 constant: optimum 0, reached exactly (the mean of J equal fp32 values is exact)
        worst = float(gap.max()) if gap.numel() else 0.0
        MEASURED["residual"] = max(MEASURED["residual"], worst)
        note(f"{tag:58s} residual: max|res-opt|/var2 = {worst:.3e} over {int(ok.sum())} frames (bound {RESIDUAL_REL:.0e})")
        assert worst <= RESIDUAL_REL, f"{tag}: sum of squared residuals misses the Procrustes optimum by {worst:.3e} var2 (> {RESIDUAL_REL:.0e})"
        assert bool((exact == 0).all()), f"{tag}: constant S2 must be reproduced exactly"
    for n in torch.nonzero(free).flatten().tolist():
        # half an fp32 ulp of the largest coordinate per point, so at most that for their mean (twice: the ulp of the next binade)
        lim = 2.0 ** -23 * float(torch.maximum(hat[n].abs().max(), ref["mu2"][n].abs().max()))
        err = float((hat[n].mean(0) - ref["mu2"][n]).abs().max())
        assert err <= lim, f"{tag} frame {n}: mean of the aligned set is {err:.3e} from mu2 (> {lim:.3e})"
        if bool(ref["s1_rank3"][n]) and float(ref["sig"][n, 0]) > 0:
            X, Y = ref["X1"][n], hat[n] - hat[n].mean(0, keepdim=True)
            A = torch.linalg.lstsq(X, Y).solution                             # Y = X A, A = s R^T
            fit = float((X @ A - Y).abs().max() / Y.abs().max())
            det = float(torch.linalg.det(A))
            assert fit <= 1e-5, f"{tag} frame {n}: the aligned set is not a linear image of S1 (fit {fit:.3e})"
            assert det > 0, f"{tag} frame {n}: det(s R) = {det:.3e}: the aligned set is not a proper similarity image of S1"
            Rm = A / det ** (1 / 3)
            orth = float((Rm @ Rm.T - torch.eye(3, dtype=torch.float64)).abs().max())
            assert orth <= 1e-4, f"{tag} frame {n}: R^T R differs from I by {orth:.3e}"


def run_sim_case(kind, N, J, device="cpu", note=print):
    S1, S2 = sim_inputs(kind, N, J)
    hat = EU.batch_compute_similarity_transform_torch(S1.to(device), S2.to(device))
    assert hat.shape == S1.shape and hat.dtype == torch.float32
    nan_frames = [True] * N if (kind == "const_s1" or J == 1) else [False] * N
    check_similarity(_njs(kind, hat), sim_reference(kind, N, J), f"similarity {kind} N={N} J={J}", note, nan_frames)


# ---- pose_errors cases --------------------------------------------------------------------------------------------------------------------------
# (kind, visibility, N, J).  Visibility: "all"; "6" / "3" / "2" / "1" visible joints per frame (another choice per frame); "no2" / "no3": that joint invisible,
# so the pelvis is half the other hip; "blank1": frame 1 (frame 0 when N = 1) has no visible joint -> MPJPE 0, PA NaN as in the reference.
POSE_CASES = [("generic", "all", N, J) for N in (1, 4, 5, 9) for J in (4, 14, 17, 64)] + [("generic", "all", 4099, 14)] + [
    ("generic", v, 5, 14) for v in ("6", "3", "2", "1", "no2", "no3", "blank1")] + [
    ("generic", "6", 9, 64), ("generic", "3", 4, 4), ("generic", "2", 9, 17), ("generic", "2", 5, 4), ("generic", "no2", 1, 4), ("generic", "no3", 9, 64),
    ("generic", "blank1", 1, 17), ("generic", "blank1", 9, 4),
    ("similarity", "all", 5, 14), ("mirrored", "all", 5, 14), ("inversion", "all", 5, 14), ("planar_s1", "all", 5, 14), ("planar_s2", "6", 5, 14),
    ("planar_both", "all", 4, 17), ("axis_s1", "all", 5, 14), ("axis_s2", "all", 5, 14), ("axis_s2", "6", 9, 64), ("axis_s2", "all", 4, 4),
    ("line_s2", "all", 5, 14), ("const_s2", "all", 5, 14), ("scale_1e-3", "all", 5, 14), ("scale_1e+3", "3", 5, 14),
]


@functools.lru_cache(maxsize=None)
def pose_inputs(kind, vis, N, J):
    """(pred (N,J,3), target (N,J,4)) CPU fp32"""
    pred, tgt = sim_inputs(kind, N, J)
    g = _gen(31 * N + J + len(vis))
    v = torch.ones(N, J)
    if vis in ("6", "3", "2", "1"):
        v = torch.zeros(N, J)
        for n in range(N):
            v[n, torch.randperm(J, generator=g)[:min(int(vis), J)]] = 1.0
    elif vis in ("no2", "no3"):
        v[:, int(vis[2:])] = 0.0
    elif vis == "blank1":
        v[min(1, N - 1)] = 0.0
    else:
        assert vis == "all", vis
    return pred.contiguous(), torch.cat([tgt, v[..., None]], dim=2)


@functools.lru_cache(maxsize=None)
def pose_reference(kind, vis, N, J):
    return pose_ref(*pose_inputs(kind, vis, N, J))


def centred_atol(pred, target):
    """masking is exact; the pelvis sum, its halving and the subtraction round to fp32 once each, on values up to twice the largest coordinate: 3 half-ulps of 2 max"""
    return 3 * 2.0 ** -23 * float(torch.maximum(pred.abs().max(), target[..., :3].abs().max()))


def run_pose_case(kind, vis, N, J, device="cpu", close=close, note=print):
    """close(name, got, ref, rtol, atol) asserts |got - ref| <= atol + rtol |ref| (and that got has no NaN)"""
    pred, tgt = pose_inputs(kind, vis, N, J)
    ref = pose_reference(kind, vis, N, J)
    tag = f"pose_errors {kind} vis={vis} N={N} J={J}"
    mpjpe, pa, pred_c, tgt_c = EU.pose_errors(pred.to(device), tgt.to(device))
    assert mpjpe.shape == (N,) and pa.shape == (N,) and pred_c.shape == (N, J, 3) and tgt_c.shape == (N, J, 3)
    ca = centred_atol(pred, tgt)
    close(f"{tag} pred_centred", pred_c, ref["pred_c"], rtol=0, atol=ca)
    close(f"{tag} target_centred", tgt_c, ref["target_c"], rtol=0, atol=ca)
    close(f"{tag} mpjpe", mpjpe, ref["mpjpe"], **SCALAR)
    pa = pa.detach().cpu().double()
    nan = torch.isnan(ref["pa"])
    if vis == "blank1":
        assert nan.tolist() == [n == min(1, N - 1) for n in range(N)], tag
        assert float(mpjpe[min(1, N - 1)]) == 0.0, tag
    else:
        assert not bool(nan.any()), tag
    assert bool(torch.isnan(pa[nan]).all()), f"{tag}: a frame without a visible joint has PA-MPJPE NaN in the reference"
    assert not bool(torch.isnan(pa[~nan]).any()), tag
    uni = ref["sim"]["unique"] & ~nan
    if bool(uni.any()):
        close(f"{tag} pa_mpjpe ({int(uni.sum())} unique frames)", pa[uni], ref["pa"][uni], **SCALAR)
    free = ~ref["sim"]["unique"] & ~nan
    if bool(free.any()):
        # rank <= 1: a mean of norms is not determined; the residual of the kernel's own alignment of the same centred sets is
        sel = torch.nonzero(free).flatten()
        pc, tc = pred_c.detach().cpu()[sel], tgt_c.detach().cpu()[sel]
        hat = EU.batch_compute_similarity_transform_torch(pc.to(device), tc.to(device))
        check_similarity(hat, similarity_ref(pc, tc), f"{tag} rank<=1 frames", note)
        # ... and PA-MPJPE is the mean joint distance of that alignment (same kernel, same centred sets)
        close(f"{tag} pa_mpjpe of the rank<=1 frames vs the aligned set", pa[sel], (hat.detach().cpu().double() - tc.double()).pow(2).sum(-1).sqrt().mean(-1), **SCALAR)


# ---- acceleration and vertex-error cases --------------------------------------------------------------------------------------------------------------
ACCEL_CASES = [(N, J) for N in (2, 3, 4, 7) for J in (1, 14, 64, 65, 70)]          # N = 2: empty result; J > 64: the joint loop strides by the wave
VERTEX_CASES = [(N, V) for N in (1, 3) for V in (1, 255, 256, 257, 6890)]           # the vertex loop strides by the 256-thread workgroup


@functools.lru_cache(maxsize=None)
def accel_inputs(N, J):
    """(joints, joints_gt, vis) -- invisible frames at the start, in the middle and at the end as far as N allows"""
    vis = torch.ones(N, dtype=torch.bool)
    vis[0] = False
    if N >= 7:
        vis[N // 2] = False
        vis[N - 1] = False
    return _randn(N, J, 3, seed=7 * N + J), _randn(N, J, 3, seed=7 * N + J + 500), vis


VIS_PATTERNS_N7 = [[0, 1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 1, 0], [1, 0, 1, 1, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0, 0]]


def run_accel_case(N, J, device="cpu", close=close):
    j, gt, vis = accel_inputs(N, J)
    tag = f"accel N={N} J={J}"
    a = EU.compute_accel(j.to(device))
    e = EU.compute_error_accel(gt.to(device), j.to(device))
    ev = EU.compute_error_accel(gt.to(device), j.to(device), vis=vis.to(device))
    assert a.shape == e.shape == (max(N - 2, 0),)
    if N < 3:
        assert ev.numel() == 0
        return
    close(f"{tag} compute_accel", a, accel_ref(j), **SCALAR)
    close(f"{tag} compute_error_accel", e, accel_ref(j, gt), **SCALAR)
    want = accel_ref(j, gt, vis)
    assert ev.shape == want.shape, (tag, ev.shape, want.shape)
    if want.numel():
        close(f"{tag} compute_error_accel vis", ev, want, **SCALAR)
    if N == 7:
        for pat in VIS_PATTERNS_N7:
            v = torch.tensor(pat, dtype=torch.bool)
            got, want = EU.compute_error_accel(gt.to(device), j.to(device), vis=v.to(device)), accel_ref(j, gt, v)
            assert got.shape == want.shape, (tag, pat, got.shape, want.shape)
            if want.numel():
                close(f"{tag} compute_error_accel vis={''.join(map(str, pat))}", got, want, **SCALAR)


def run_vertex_case(N, V, device="cpu", close=close):
    a, b = _randn(N, V, 3, seed=3 * V + N), _randn(N, V, 3, seed=3 * V + N + 1)
    got = EU.compute_error_verts(pred_verts=a.to(device), target_verts=b.to(device))
    assert got.shape == (N,)
    close(f"vertex error N={N} V={V}", got, vertex_ref(a, b), **SCALAR)


# ---- the C entry points on guarded buffers -----------------------------------------------------------------------------------------------------------
class Guarded:
    """a float tensor of `shape` between two guard zones, all of it -- the window too -- filled with the sentinel byte"""

    def __init__(self, shape, device):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((4 * n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.t = self.buf[GUARD:GUARD + 4 * n].view(torch.float32).view(shape)

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.cpu() == SENTINEL).all())


def run_guarded_calls(device="cpu", close=close):
    """the four entry points through the C interface at N = 5, J = 14 (acceleration also N = 3, J = 65), inputs allocated at exactly their size, every output a
    window in a sentinel-filled buffer: the window holds the fp64 reference's values and the bytes before and after it come back bit for bit"""
    lib, p, st = L.lib(), ops._p, ops._stream
    N, J = 5, 14
    pred, tgt = (t.clone().to(device) for t in pose_inputs("generic", "6", N, J))
    ref = pose_reference("generic", "6", N, J)
    outs = dict(mpjpe=Guarded((N,), device), pa_mpjpe=Guarded((N,), device), pred_centred=Guarded((N, J, 3), device), target_centred=Guarded((N, J, 3), device))
    rc = lib.maed_eval_pose_errors(p(pred), p(tgt), N, J, *(p(g.t) for g in outs.values()), st())
    assert rc == 0, lib.maed_last_error()
    close("guarded pose_errors mpjpe", outs["mpjpe"].t, ref["mpjpe"], **SCALAR)
    close("guarded pose_errors pa_mpjpe", outs["pa_mpjpe"].t, ref["pa"], **SCALAR)
    ca = centred_atol(pred.cpu(), tgt.cpu())
    close("guarded pose_errors pred_centred", outs["pred_centred"].t, ref["pred_c"], rtol=0, atol=ca)
    close("guarded pose_errors target_centred", outs["target_centred"].t, ref["target_c"], rtol=0, atol=ca)
    for name, g in outs.items():
        assert g.guards_intact(), f"maed_eval_pose_errors wrote outside {name}"

    S1, S2 = (t.clone().to(device) for t in sim_inputs("generic", N, J))
    hat = Guarded((N, J, 3), device)
    rc = lib.maed_similarity_transform(p(S1), p(S2), N, J, p(hat.t), st())
    assert rc == 0, lib.maed_last_error()
    check_similarity(hat.t, sim_reference("generic", N, J), "guarded similarity_transform")
    assert hat.guards_intact(), "maed_similarity_transform wrote outside S1_hat"

    for n, j in ((5, 14), (3, 65)):
        jn, gt, _ = (t.clone().to(device) for t in accel_inputs(n, j))
        for with_gt in (False, True):
            out = Guarded((n - 2,), device)                  # N - 2 entries, not N
            rc = lib.maed_eval_accel(p(jn), p(gt) if with_gt else None, n, j, p(out.t), st())
            assert rc == 0, lib.maed_last_error()
            close(f"guarded eval_accel N={n} J={j} gt={with_gt}", out.t, accel_ref(jn.cpu(), gt.cpu() if with_gt else None), **SCALAR)
            assert out.guards_intact(), f"maed_eval_accel N={n} J={j} wrote outside its N-2 outputs"

    a, b = _randn(N, 257, 3, seed=11).to(device), _randn(N, 257, 3, seed=12).to(device)
    out = Guarded((N,), device)
    rc = lib.maed_eval_vertex_error(p(a), p(b), N, 257, p(out.t), st())
    assert rc == 0, lib.maed_last_error()
    close("guarded eval_vertex_error N=5 V=257", out.t, vertex_ref(a.cpu(), b.cpu()), **SCALAR)
    assert out.guards_intact(), "maed_eval_vertex_error wrote outside its outputs"


ERR_ARG, ERR_SHAPE = -1, -2          # include/maed_hip.h maed_status


def run_argument_checks(device="cpu"):
    """bad extents and null pointers return their status and launch nothing (every output still holds the sentinel); N = 0 is MAED_OK and launches nothing either"""
    lib, p, st = L.lib(), ops._p, ops._stream

    def call(fn, want, *args, outs):
        rc = fn(*args, st())
        assert rc == want, f"{fn.__name__}{args[2:4]} returned {rc}, expected {want}: {lib.maed_last_error()}"
        for g in outs:
            assert g.untouched(), f"{fn.__name__}{args[2:4]} -> {rc} wrote to an output"

    N = 5
    for J in (3, 65):
        pred, tgt = torch.zeros(N, J, 3, device=device), torch.ones(N, J, 4, device=device)
        o = [Guarded((N,), device), Guarded((N,), device), Guarded((N, J, 3), device), Guarded((N, J, 3), device)]
        call(lib.maed_eval_pose_errors, ERR_SHAPE, p(pred), p(tgt), N, J, *(p(g.t) for g in o), outs=o)
    J = 65
    S1, S2, hat = torch.ones(N, J, 3, device=device), torch.ones(N, J, 3, device=device), Guarded((N, J, 3), device)
    call(lib.maed_similarity_transform, ERR_SHAPE, p(S1), p(S2), N, J, p(hat.t), outs=[hat])
    call(lib.maed_similarity_transform, ERR_SHAPE, p(S1), p(S2), N, 0, p(hat.t), outs=[hat])
    J = 14
    pred, tgt = torch.zeros(N, J, 3, device=device), torch.ones(N, J, 4, device=device)
    o = [Guarded((N,), device), Guarded((N,), device), Guarded((N, J, 3), device), Guarded((N, J, 3), device)]
    ptrs = [p(pred), p(tgt), N, J] + [p(g.t) for g in o]
    for k in (0, 1, 4, 5):                                   # pred, target, mpjpe, pa_mpjpe (the two centred outputs are optional)
        a = list(ptrs)
        a[k] = None
        call(lib.maed_eval_pose_errors, ERR_ARG, *a, outs=o)
    call(lib.maed_eval_pose_errors, 0, p(pred), p(tgt), 0, J, *(p(g.t) for g in o), outs=o)
    S1, hat = torch.ones(N, J, 3, device=device), Guarded((N, J, 3), device)
    for a in ([None, p(S1), N, J, p(hat.t)], [p(S1), None, N, J, p(hat.t)], [p(S1), p(S1), N, J, None]):
        call(lib.maed_similarity_transform, ERR_ARG, *a, outs=[hat])
    call(lib.maed_similarity_transform, 0, p(S1), p(S1), 0, J, p(hat.t), outs=[hat])
    out = Guarded((N,), device)
    call(lib.maed_eval_accel, ERR_ARG, None, None, N, J, p(out.t), outs=[out])
    call(lib.maed_eval_accel, ERR_ARG, p(S1), None, N, J, None, outs=[out])
    call(lib.maed_eval_accel, ERR_SHAPE, p(S1), None, N, 0, p(out.t), outs=[out])
    call(lib.maed_eval_accel, 0, p(S1), None, 0, J, p(out.t), outs=[out])
    call(lib.maed_eval_accel, 0, p(S1), None, 2, J, p(out.t), outs=[out])          # fewer than three frames: no window
    call(lib.maed_eval_vertex_error, ERR_ARG, None, p(S1), N, J, p(out.t), outs=[out])
    call(lib.maed_eval_vertex_error, ERR_ARG, p(S1), None, N, J, p(out.t), outs=[out])
    call(lib.maed_eval_vertex_error, ERR_ARG, p(S1), p(S1), N, J, None, outs=[out])
    call(lib.maed_eval_vertex_error, ERR_SHAPE, p(S1), p(S1), N, 0, p(out.t), outs=[out])
    call(lib.maed_eval_vertex_error, 0, p(S1), p(S1), 0, J, p(out.t), outs=[out])


# ---- wrapper level ---------------------------------------------------------------------------------------------------------------------------------
def run_target_vertices_chunks(device="cpu"):
    """target_vertices in chunks of 3 (7 = 3 + 3 + 1 frames) equals the single chunk bit for bit"""
    from maed_amd.smpl import SMPL
    smpl = SMPL().to(device)
    theta = (_randn(7, 85, seed=41) * 0.3).to(device)
    whole, parts = EU.target_vertices(theta, smpl), EU.target_vertices(theta, smpl, chunk=3)
    assert whole.shape == parts.shape == (7, 6890, 3)
    assert torch.equal(whole, parts)


def run_evaluator(device="cpu", close=close):
    """Evaluator.evaluate() on accumulators from the generators above (N = 9, J = 14, mixed visibility, synthetic SMPL) against the five fp64 means.  The
    target vertices are the product's own (SMPL is not an evaluation kernel): the reference takes the vertex kernel's fp32 inputs like every other"""
    from maed_amd.evaluate import Evaluator
    from maed_amd.smpl import SMPL
    N, J = 9, 14
    pred, tgt = pose_inputs("generic", "all", N, J)
    tgt = tgt.clone()
    for n, v in enumerate(("all", "6", "3", "no2", "no3", "2", "all", "6", "no2")):       # mixed visibility, every frame with a unique alignment
        tgt[n, :, 3] = pose_inputs("generic", v, 5, J)[1][n % 5, :, 3]
    theta = _randn(N, 85, seed=43) * 0.3
    smpl = SMPL().to(device)
    tv = EU.target_vertices(theta.to(device), smpl)
    pv = tv.cpu() + 0.05 * _randn(N, 6890, 3, seed=44)
    ev = Evaluator()
    ev.smpl = smpl
    half = N // 2                                                                          # two batches: evaluate() concatenates
    for sl in (slice(0, half), slice(half, N)):
        for k, v in (("pred_j3d", pred), ("target_j3d", tgt), ("pred_verts", pv), ("target_theta", theta)):
            ev.evaluation_accumulators[k].append(v[sl].clone().to(device))
    eval_dict, num_pred = ev.evaluate()
    assert num_pred == N and list(eval_dict) == ["mpjpe", "pa-mpjpe", "pve", "accel", "accel_err"]
    ref = pose_ref(pred, tgt)
    assert bool(ref["sim"]["unique"].all())
    want = {"mpjpe": ref["mpjpe"].mean(), "pa-mpjpe": ref["pa"].mean(), "pve": vertex_ref(pv, tv.cpu()).mean(), "accel": accel_ref(ref["pred_c"]).mean(),
            "accel_err": accel_ref(ref["pred_c"], ref["target_c"]).mean()}
    for k, w in want.items():
        close(f"Evaluator.evaluate {k} (mm)", torch.tensor([eval_dict[k]], dtype=torch.float64), (w * 1000).reshape(1), rtol=SCALAR["rtol"], atol=SCALAR["atol"] * 1000)
