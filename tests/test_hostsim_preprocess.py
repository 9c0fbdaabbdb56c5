"""csrc/preprocess.hip on the host simulator (tests/_hostsim_preprocess.py): every stage after the warp against the reference's recorded outputs
(tests/golden/g16_clip_preprocess.npz, written by scripts/make_golden_preprocess.py), the three launch forms against each other, the warp against its fp64
definition (also for regions flush with every border of a larger buffer), a record sent through a DataLoader worker, and one run under AddressSanitizer.

Tolerances: the normalised output of a given uint8 patch is bit-equal (three correctly rounded fp32 operations); erase, flip, brightness, saturation,
contrast and hue are equal in uint8 (the numpy restatement of tests/_preprocess_ref.py reproduces g16 with zero differing pixel-channels, hue included --
test_restatement_reproduces_g16 measures it -- so by the rule of docs/design/10_preprocess.md the kernel's bound is exact equality); the warp may differ
from its fp64 definition by one level (fp32 coordinates can only flip rounding ties at < 1024 px)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _hostsim_preprocess as S
import _preprocess_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DIRECT, LDS, TWO = 1, 2, 3


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_clip_preprocess")


def expect(u8_frames):
    return np.stack([R.normalise_f32(f) for f in u8_frames])


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, what
    diff = got.view(np.uint32) != ref.view(np.uint32)
    if diff.any():
        lv = np.abs(R.to_levels(got) - R.to_levels(ref))
        print(f"{what}: {int(diff.sum())} of {diff.size} values differ; max level difference {lv.max()}, share {np.mean(lv > 0):.5f}")
    assert not diff.any(), what


def set_clip(t, n, order=(), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, flip=False):
    from maed_amd import data as D
    t["clip_i"][n, 0] = int(flip)
    t["clip_i"][n, 1:5] = 0
    t["clip_i"][n, 1:1 + len(order)] = order
    t["clip_i"][n, 5] = D.hue_shift_levels(hue)
    t["clip_f"][n] = (brightness, saturation, 0.0, contrast)


def test_restatement_reproduces_g16(g16):
    """the measurement the hue bound rests on: the test file's own restatement against the reference's outputs, all 24 orders and every operation alone"""
    worst, share = 0, 0.0
    for i, (order, f) in enumerate(zip(g16["jit_orders"], g16["jit_factors"])):
        src = (g16["patch_a"], g16["patch_b"])[i % 2][(i // 2) % 2]
        ref = (g16["jit_out_a"], g16["jit_out_b"])[i % 2][i // 2]
        got = R.jitter_u8(src, list(order), brightness=f[0], contrast=f[1], saturation=f[2], shift=int(f[3] * 255) & 255)
        d = np.abs(got.astype(int) - ref.astype(int))
        worst, share = max(worst, d.max()), max(share, float(np.mean(d > 0)))
    for k, (code, fv) in enumerate(g16["single_ops"]):
        for t in range(2):
            got = R.jitter_u8(g16["patch_b"][t], [int(code)], brightness=fv, saturation=fv, contrast=fv, shift=int(fv * 255) & 255)
            d = np.abs(got.astype(int) - g16["single_out"][k, t].astype(int))
            worst, share = max(worst, d.max()), max(share, float(np.mean(d > 0)))
    print(f"restatement vs g16: max level difference {worst}, largest share of differing pixel-channels {share:.5f}")
    assert worst == 0 and share == 0.0


def test_normalise_bit_equal(g16):
    t = R.identity_tables(list(g16["patch_b"]))
    for form in (DIRECT, LDS, TWO):
        assert_bits(S.run(t, 56, 56, form), g16["norm_out"], f"normalise, form {form}")


@pytest.mark.parametrize("form", [LDS, TWO])
def test_every_jitter_order(g16, form):
    for half, key in ((0, "a"), (1, "b")):
        idx = [i for i in range(24) if i % 2 == half]
        patches = [g16["patch_" + key][(i // 2) % 2] for i in idx]
        t = R.identity_tables(patches, clip_of=list(range(len(idx))), n_clips=len(idx))
        for n, i in enumerate(idx):
            f = g16["jit_factors"][i]
            set_clip(t, n, [int(o) for o in g16["jit_orders"][i]], brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3])
        H, W = patches[0].shape[:2]
        assert_bits(S.run(t, H, W, form), expect(g16["jit_out_" + key]), f"24 jitter orders, clip {key}, form {form}")


def test_each_operation_alone(g16):
    for k, (code, fv) in enumerate(g16["single_ops"]):
        code = int(code)
        t = R.identity_tables(list(g16["patch_b"]))
        set_clip(t, 0, [code], brightness=fv, contrast=fv, saturation=fv, hue=fv)
        for form in ((LDS, TWO) if code == 4 else (DIRECT, LDS, TWO)):
            assert_bits(S.run(t, 56, 56, form), expect(g16["single_out"][k]), f"operation {code} factor {fv} form {form}")


def test_erase_all_four_sides(g16):
    from maed_amd import data as D
    aug = D.ClipAugment(64, 48)
    for side in range(4):
        rec = D.ClipParams(bboxes=np.zeros((2, 4)), erase_side=side, erase_ratio=g16["erase_ratios"][side])
        t = R.identity_tables(list(g16["patch_a"]))
        t["frame_i"][:, 5:7] = aug.erase_rows(rec)
        for form in (DIRECT, LDS, TWO):
            assert_bits(S.run(t, 64, 48, form), expect(g16["erase_out"][side]), f"erase side {side} form {form}")


def test_flip(g16):
    t = R.identity_tables(list(g16["patch_a"]))
    set_clip(t, 0, flip=True)
    for form in (DIRECT, LDS, TWO):
        assert_bits(S.run(t, 64, 48, form), expect(g16["flip_out"]), f"flip form {form}")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_whole_chain_after_the_warp(g16, tag):
    from maed_amd import data as D
    patches = g16["patch_" + tag]
    H, W = patches.shape[1:3]
    f = g16[f"chain_{tag}_factors"]
    side, *ratios = g16[f"chain_{tag}_erase"]
    rec = D.ClipParams(bboxes=np.zeros((2, 4)), erase_side=int(side), erase_ratio=np.array(ratios))
    t = R.identity_tables(list(patches))
    set_clip(t, 0, [int(o) for o in g16[f"chain_{tag}_order"]], brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3], flip=True)
    t["frame_i"][:, 5:7] = D.ClipAugment(H, W).erase_rows(rec)
    for form in (LDS, TWO):
        assert_bits(S.run(t, H, W, form), g16[f"chain_{tag}_out"], f"chain {tag} form {form}")


def test_forms_agree_and_warp_matches_fp64_through_the_python_layer():
    """pack_clips -> preprocess_clips on the simulator: jittered clips in the LDS and the two-launch form (bit-equal; their values are checked by
    test_warp_with_jitter_agrees_where_the_patch_agrees); plain clips in all three forms, bit-equal and within the warp's one level of the fp64 definition"""
    from maed_amd import data as D
    H, W = 24, 32
    aug = D.ClipAugment(H, W)
    for jitter, forms in ((True, (LDS, TWO)), (False, (DIRECT, LDS, TWO))):
        frames, records = R.random_scene(5 + jitter, 3, 2, H, W, lo=20, hi=300, jitter=jitter)
        packed = D.pack_clips(frames, records, aug)
        with S.patched():
            outs = [D.preprocess_clips(packed, device="cpu", form=f).numpy() for f in forms]
        assert outs[0].shape == (3, 2, 3, H, W) and outs[0].dtype == np.float32
        for o in outs[1:]:
            assert_bits(o, outs[0], f"forms {forms}, jitter={jitter}")
        if not jitter:
            ref, _ = R.packed_reference(packed)
            d = np.abs(R.to_levels(outs[0].reshape(ref.shape)) - R.to_levels(ref))
            print(f"warp vs fp64: max level difference {d.max()}, share {np.mean(d > 0):.5f}")
            assert d.max() <= 1


def border_tables(with_nan):
    """regions flush with the left / top / right / bottom edge of a 40 x 52 image (the first and the last byte of the packed buffer included), sampled from well
    outside on every side, with weight on the border pixels: a tap one pixel past any edge of a region lands on a neighbouring pixel of this noise image"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)
    cases = [(0, 0, 52, 40, (4.0, 0, -6.0, 0, 3.0, -5.0)), (0, 0, 1, 40, (0.5, 0, -3.0, 0, 3.0, -2.0)), (51, 39, 1, 1, (0.3, 0.1, -2.0, -0.1, 0.3, -2.0)),
             (10, 39, 42, 1, (3.0, 0.5, -4.0, 0.2, 0.2, -1.5)), (3, 5, 20, 10, (1.7, 0.0, -2.3, 0.0, 0.9, -1.4)), (30, 0, 22, 40, (1.9, 0.3, -3.1, -0.2, 2.9, -2.2))]
    if with_nan:
        cases.append((0, 0, 52, 40, (1e9, 0, -1e9, 0, float("nan"), 0)))
    fi = np.array([[(y0 * 52 + x0) * 3, h, w, 52 * 3, 0, 0, 0, 0] for x0, y0, w, h, _ in cases], np.int32)
    fm = np.array([m for *_, m in cases], np.float32)
    t = dict(src=img.reshape(-1).copy(), frame_i=fi, frame_minv=fm, clip_i=np.zeros((1, 8), np.int32), clip_f=np.array([[1, 1, 0, 1]], np.float32))
    regions = [img[y0:y0 + h, x0:x0 + w] for x0, y0, w, h, _ in cases]
    return t, regions


def test_regions_flush_with_every_border_match_the_fp64_definition():
    """the out-of-range gather: every region here is a window INSIDE a larger buffer, so a tap past its right / bottom / left / top edge reads a valid but wrong
    pixel (no sanitizer can see that); the values can"""
    t, regions = border_tables(with_nan=False)
    H = W = 16
    got = S.run(t, H, W, DIRECT)
    worst = 0
    for f, region in enumerate(regions):
        ref = R.normalise_f32(R.warp_fp64(region, t["frame_minv"][f].astype(np.float64), H, W))
        d = np.abs(R.to_levels(got[f]) - R.to_levels(ref))
        worst = max(worst, d.max())
        assert d.max() <= 1, (f, d.max())
        assert R.warp_fp64(region, t["frame_minv"][f].astype(np.float64), H, W).any(), f      # (the case samples something: not a vacuous all-zero patch)
    print(f"border regions vs fp64: max level difference {worst}")
    for form in (LDS, TWO):
        assert_bits(S.run(t, H, W, form), got, f"border regions form {form}")


def test_packed_clips_through_a_loader_worker():
    """the documented integration: a DataLoader worker's collate function calls pack_clips (no GPU runtime in the worker), the record arrives in the main
    process through the loader's transport, its tables are still views of the one buffer, and it runs"""
    import torch
    from maed_amd import data as D
    H, W = 16, 16

    loader = torch.utils.data.DataLoader(_Scenes(), batch_size=2, num_workers=1, collate_fn=_collate)
    packed = next(iter(loader))
    assert isinstance(packed, D.PackedClips) and (packed.N, packed.T) == (2, 2) and not torch.cuda.is_initialized()
    local = _collate([_Scenes()[0], _Scenes()[1]])
    assert torch.equal(packed.blob, local.blob)
    assert np.shares_memory(packed.clip_f, packed.blob.numpy()) and np.shares_memory(packed.frame_i, packed.blob.numpy())
    with S.patched():
        a = D.preprocess_clips(packed, device="cpu").numpy()
        b = D.preprocess_clips(local, device="cpu").numpy()
        assert_bits(a, b, "through the loader vs packed here")
        # a field set by hand AFTER transport is what the kernel reads
        packed.clip_i[:, 0] ^= 1
        c = D.preprocess_clips(packed, device="cpu").numpy()
    assert_bits(c, np.ascontiguousarray(a[..., ::-1]), "flip flag set after transport")


class _Scenes:
    def __len__(self):
        return 2

    def __getitem__(self, i):
        frames, records = R.random_scene(40 + i, 1, 2, 16, 16, lo=20, hi=200, jitter=False)
        return frames[0], records[0]


def _collate(items):
    from maed_amd import data as D
    return D.pack_clips([f for f, _ in items], [r for _, r in items], D.ClipAugment(16, 16))


def test_warp_with_jitter_agrees_where_the_patch_agrees():
    """with jitter downstream a one-level warp tie is amplified by the blends, so the jittered output is checked from the kernel's OWN uint8 patch: warp-only
    run -> levels -> restatement of the rest == the full run, bit for bit"""
    from maed_amd import data as D
    H, W = 24, 32
    frames, records = R.random_scene(11, 2, 2, H, W, lo=20, hi=300, jitter=True)
    packed = D.pack_clips(frames, records, D.ClipAugment(H, W))
    plain = D.pack_clips(frames, [D.ClipParams(bboxes=r.bboxes, scale=r.scale, rot=r.rot, shift=r.shift) for r in records], D.ClipAugment(H, W))
    with S.patched():
        full = D.preprocess_clips(packed, device="cpu").numpy().reshape(4, 3, H, W)
        warp = D.preprocess_clips(plain, device="cpu").numpy().reshape(4, 3, H, W)
    patches = R.to_levels(warp).transpose(0, 2, 3, 1).astype(np.uint8)
    ref = []
    for f in range(4):
        ci, cf = packed.clip_i[f // 2], packed.clip_f[f // 2]
        ref.append(R.chain_ref(patches[f], [int(o) for o in ci[1:5] if o], cf[0], cf[1], cf[3], int(ci[5]), int(packed.frame_i[f, 5]), int(packed.frame_i[f, 6]), bool(ci[0])))
    assert_bits(full, np.stack(ref), "full chain from the kernel's own patch")


def test_refusals():
    t = R.identity_tables([np.zeros((8, 8, 3), np.uint8)])
    t["clip_i"][0, 1] = 4
    with pytest.raises(RuntimeError, match="direct form"):
        S.run(t, 8, 8, DIRECT)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        S.run(R.identity_tables([np.zeros((8, 6, 3), np.uint8)]), 8, 6)
    with pytest.raises(RuntimeError, match="does not fit"):
        S.run(R.identity_tables([np.zeros((256, 256, 3), np.uint8)]), 256, 256, LDS)


ASAN_JOB = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import _hostsim_preprocess as S
from test_hostsim_preprocess import border_tables
t, _ = border_tables(with_nan=True)
t["frame_i"][:, 5] = 2
t["clip_i"][0] = (1, 2, 4, 3, 1, 40, 0, 0)
t["clip_f"][0] = (1.2, 0.8, 0, 1.1)
H = W = 16
a = S.run(t, H, W, 2)
b = S.run(t, H, W, 3)
assert (a.view(np.uint32) == b.view(np.uint32)).all()
t["clip_i"][0, 1:5] = 0
S.run(t, H, W, 1)
print("ASAN_JOB_DONE")
"""


def test_no_out_of_bounds_access_under_address_sanitizer(tmp_path):
    clang = os.environ.get("MAED_HOST_CXX", "/opt/rocm/lib/llvm/bin/clang++")
    rt = subprocess.run([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    assert os.path.isabs(rt) and os.path.exists(rt), "no AddressSanitizer runtime next to " + clang
    log = str(tmp_path / "asan")
    env = dict(os.environ, MAED_SIM_ASAN="1", LD_PRELOAD=rt, ASAN_OPTIONS=f"detect_leaks=0:halt_on_error=0:log_path={log}:detect_odr_violation=0")
    r = subprocess.run([sys.executable, "-c", ASAN_JOB % (os.path.dirname(HERE), HERE)], env=env, capture_output=True, text=True, timeout=600)
    reports = "".join(open(os.path.join(tmp_path, f), errors="replace").read() for f in os.listdir(tmp_path))
    assert "ERROR: AddressSanitizer" not in reports and "ERROR: AddressSanitizer" not in r.stderr, (reports + r.stderr)[-4000:]
    assert r.returncode == 0 and "ASAN_JOB_DONE" in r.stdout, (r.stdout + r.stderr)[-4000:]
