"""csrc/preprocess.hip on the MI355X, through ctypes (maed_amd.ops.clip_preprocess / maed_amd.data.preprocess_clips), reading only tests/golden:
g16 stage by stage, the evaluation fast path, 8 x 16 frames at 224 x 224 and 2 x 64 frames at 256 x 256 from a seeded generator, the LDS form against the
two-launch form, the hand-over to MAED.forward, and one negative test per refusal.

Tolerances (docs/design/10_preprocess.md): normalised output of a given uint8 patch bit-equal; erase / flip / brightness / saturation / contrast / hue equal
in uint8 against g16 (the restatement of tests/_preprocess_ref.py reproduces g16 exactly, hue included, so the kernel's bound is exact equality); the warp at
most one level from its fp64 definition (coordinates < 1024 px).  Because a one-level rounding tie of the warp is multiplied by the blends behind it, a
jittered clip is compared in two steps that together cover the chain: the kernel's warp alone against fp64 (one level), and the full run against the
restatement applied to the kernel's OWN uint8 patch (bit-equal)."""
import numpy as np
import pytest
import torch

import _preprocess_ref as R
from _util import note

pytestmark = [pytest.mark.gpu]
DIRECT, LDS, TWO = 1, 2, 3


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_clip_preprocess")


def run_gpu(t, H, W, form=0):
    from maed_amd import ops
    parts = [np.ascontiguousarray(t[k]).view(np.uint8).reshape(-1) for k in ("frame_i", "frame_minv", "clip_i", "clip_f")]
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at += p.size
    px = (at + 255) // 256 * 256
    blob = np.zeros(px + t["src"].size, dtype=np.uint8)
    for o, p in zip(offs, parts):
        blob[o:o + p.size] = p
    blob[px:] = t["src"]
    F, N = len(t["frame_i"]), len(t["clip_i"])
    out = torch.full((F, 3, H, W), float("nan"), device="cuda")
    ops.clip_preprocess(torch.from_numpy(blob).cuda(), (*offs, px), t["src"].size, F, N, H, W, R.MEAN, R.STD, bool((t["clip_i"][:, 1:5] == 4).any()), out, form)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_bits(got, ref, what):
    assert got.shape == ref.shape, what
    diff = got.view(np.uint32) != ref.view(np.uint32)
    lv = np.abs(R.to_levels(got) - R.to_levels(ref)) if diff.any() else np.zeros(1)
    note(f"preprocess {what:64s} differing values {int(diff.sum())}/{diff.size} max level diff {lv.max()} share {np.mean(lv > 0):.5f}")
    assert not diff.any(), what


def expect(u8_frames):
    return np.stack([R.normalise_f32(f) for f in u8_frames])


def set_clip(t, n, order=(), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, flip=False):
    from maed_amd import data as D
    t["clip_i"][n, 0] = int(flip)
    t["clip_i"][n, 1:5] = 0
    t["clip_i"][n, 1:1 + len(order)] = order
    t["clip_i"][n, 5] = D.hue_shift_levels(hue)
    t["clip_f"][n] = (brightness, saturation, 0.0, contrast)


def test_g16_normalise_and_eval_fast_path(g16):
    t = R.identity_tables(list(g16["patch_b"]))
    for form in (0, DIRECT, LDS, TWO):          # 0 resolves to the direct form: no jitter, no erase, no flip = the evaluation path, nothing staged
        assert_bits(run_gpu(t, 56, 56, form), g16["norm_out"], f"g16 normalise form {form}")


@pytest.mark.parametrize("form", [0, LDS, TWO])
def test_g16_every_jitter_order(g16, form):
    for half, key in ((0, "a"), (1, "b")):
        idx = [i for i in range(24) if i % 2 == half]
        patches = [g16["patch_" + key][(i // 2) % 2] for i in idx]
        t = R.identity_tables(patches, clip_of=list(range(len(idx))), n_clips=len(idx))
        for n, i in enumerate(idx):
            f = g16["jit_factors"][i]
            set_clip(t, n, [int(o) for o in g16["jit_orders"][i]], brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3])
        H, W = patches[0].shape[:2]
        assert_bits(run_gpu(t, H, W, form), expect(g16["jit_out_" + key]), f"g16 24 jitter orders clip {key} form {form}")


def test_g16_each_operation_alone(g16):
    for k, (code, fv) in enumerate(g16["single_ops"]):
        code = int(code)
        t = R.identity_tables(list(g16["patch_b"]))
        set_clip(t, 0, [code], brightness=fv, contrast=fv, saturation=fv, hue=fv)
        for form in ((LDS, TWO) if code == 4 else (DIRECT, LDS, TWO)):
            assert_bits(run_gpu(t, 56, 56, form), expect(g16["single_out"][k]), f"g16 operation {code} factor {fv} form {form}")


def test_g16_erase_flip_and_whole_chain(g16):
    from maed_amd import data as D
    aug = D.ClipAugment(64, 48)
    for side in range(4):
        rec = D.ClipParams(bboxes=np.zeros((2, 4)), erase_side=side, erase_ratio=g16["erase_ratios"][side])
        t = R.identity_tables(list(g16["patch_a"]))
        t["frame_i"][:, 5:7] = aug.erase_rows(rec)
        for form in (DIRECT, LDS, TWO):
            assert_bits(run_gpu(t, 64, 48, form), expect(g16["erase_out"][side]), f"g16 erase side {side} form {form}")
    t = R.identity_tables(list(g16["patch_a"]))
    set_clip(t, 0, flip=True)
    for form in (DIRECT, LDS, TWO):
        assert_bits(run_gpu(t, 64, 48, form), expect(g16["flip_out"]), f"g16 flip form {form}")
    for tag in ("a", "b"):
        patches = g16["patch_" + tag]
        H, W = patches.shape[1:3]
        f = g16[f"chain_{tag}_factors"]
        side, *ratios = g16[f"chain_{tag}_erase"]
        rec = D.ClipParams(bboxes=np.zeros((2, 4)), erase_side=int(side), erase_ratio=np.array(ratios))
        t = R.identity_tables(list(patches))
        set_clip(t, 0, [int(o) for o in g16[f"chain_{tag}_order"]], brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3], flip=True)
        t["frame_i"][:, 5:7] = D.ClipAugment(H, W).erase_rows(rec)
        for form in (0, LDS, TWO):
            assert_bits(run_gpu(t, H, W, form), g16[f"chain_{tag}_out"], f"g16 chain {tag} form {form}")


@pytest.mark.parametrize("n_clips,T,size", [(8, 16, 224), (2, 64, 256)])
def test_seeded_clips_against_the_fp64_definition(n_clips, T, size):
    from maed_amd import data as D
    from maed_amd import ops
    aug = D.ClipAugment(size, size)
    frames, records = R.random_scene(100 + size, n_clips, T, size, size, lo=100, hi=900, jitter=True)
    plain = [D.ClipParams(bboxes=r.bboxes, scale=r.scale, rot=r.rot, shift=r.shift) for r in records]
    packed, packed_plain = D.pack_clips(frames, records, aug), D.pack_clips(frames, plain, aug)
    sides = np.sqrt(packed.frame_i[:, 1].astype(np.float64) * packed.frame_i[:, 2])
    note(f"preprocess {n_clips} x {T} at {size}: region sides {sides.min():.0f} .. {sides.max():.0f} px, {packed.src_bytes / 1e6:.1f} MB packed")
    F = n_clips * T
    warp = D.preprocess_clips(packed_plain)
    full = D.preprocess_clips(packed)
    assert full.shape == (n_clips, T, 3, size, size) and full.dtype == torch.float32 and full.is_contiguous() and full.is_cuda
    two = D.preprocess_clips(packed, form=ops.PRE_FORM_TWO)
    torch.cuda.synchronize()
    warp, full, two = (x.cpu().numpy().reshape(F, 3, size, size) for x in (warp, full, two))
    # 1. the warp against its fp64 definition: at most one level anywhere
    ref, _ = R.packed_reference(packed_plain)
    d = np.abs(R.to_levels(warp) - R.to_levels(ref))
    note(f"preprocess warp vs fp64 at {size}: max level difference {d.max()}, share of differing pixel-channels {np.mean(d > 0):.6f}")
    assert d.max() <= 1
    # 2. everything behind the warp from the kernel's own uint8 patch: bit-equal
    patches = R.to_levels(warp).transpose(0, 2, 3, 1).astype(np.uint8)
    rest = []
    for f in range(F):
        ci, cf = packed.clip_i[f // T], packed.clip_f[f // T]
        rest.append(R.chain_ref(patches[f], [int(o) for o in ci[1:5] if o], cf[0], cf[1], cf[3], int(ci[5]), int(packed.frame_i[f, 5]), int(packed.frame_i[f, 6]), bool(ci[0])))
    assert_bits(full, np.stack(rest), f"{n_clips} x {T} at {size}: chain behind the kernel's own patch")
    # 3. the forms agree (the automatic choice for a jittered clip is the two-launch form; at 224 the LDS form fits and is compared too)
    assert_bits(two, full, f"{n_clips} x {T} at {size}: two-launch form vs automatic form")
    if size == 224:
        lds = D.preprocess_clips(packed, form=ops.PRE_FORM_LDS).cpu().numpy().reshape(F, 3, size, size)
        assert_bits(lds, two, "224: LDS form vs two-launch form")
        direct = D.preprocess_clips(packed_plain, form=ops.PRE_FORM_LDS).cpu().numpy().reshape(F, 3, size, size)
        assert_bits(direct, warp, "224: evaluation path, LDS form vs direct form")


def test_output_feeds_maed_forward_without_copy_or_cast():
    import maed_amd
    from maed_amd import data as D
    aug = D.ClipAugment(64, 64, color_jitter=0.3, erase_prob=0.3, seed=2)
    frames, _ = R.random_scene(9, 2, 4, 64, 64, lo=60, hi=300, jitter=False)
    records = [aug.sample(np.tile([300., 250., 120., 160.], (4, 1))) for _ in range(2)]
    clip = D.preprocess_clips(D.pack_clips(frames, records, aug))
    assert clip.shape == (2, 4, 3, 64, 64) and clip.dtype == torch.float32 and clip.is_contiguous() and clip.is_cuda
    m = maed_amd.MAED(num_blocks=2, num_heads=2, embed_dim=128, hidden_dim=64, img_size=64, compute_dtype=torch.float32).to("cuda").eval()
    before = clip.clone()
    with torch.no_grad():
        out = m(clip)
    assert all(torch.isfinite(out[k]).all() for k in ("theta", "kp_3d")) and torch.equal(clip, before)
    # into a caller's buffer and on a caller's stream
    s = torch.cuda.Stream()
    buf = torch.empty_like(clip)
    got = D.preprocess_clips(D.pack_clips(frames, records, aug), out=buf, stream=s)
    assert got.data_ptr() == buf.data_ptr() and torch.equal(buf, clip)          # (torch.equal runs on the current stream: ordered by preprocess_clips)


def test_side_stream_result_is_ordered_for_the_current_stream():
    """stream=s: the result is consumed on the default stream at once, with no event and no host synchronise in between, many times over so that the side
    stream's blocks are recycled while consumers may still be reading: every consumer must see the finished clip (preprocess_clips makes the current stream wait
    for s and records the result there).  The sums are compared only after everything was queued."""
    from maed_amd import data as D
    aug = D.ClipAugment(224, 224)
    side = torch.cuda.Stream()
    scenes = []
    for k in range(3):
        frames, records = R.random_scene(60 + k, 4, 4, 224, 224, lo=100, hi=600, jitter=True)
        scenes.append(D.pack_clips(frames, records, aug, pin=True))
    want = [D.preprocess_clips(p).double().sum() for p in scenes]
    ballast = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    got = []
    for i in range(12):
        p = scenes[i % 3]
        ballast = ballast @ ballast * 1e-4                                   # keeps the default stream busy: the side stream runs ahead of it
        clip = D.preprocess_clips(p, stream=side)
        got.append((i % 3, clip.double().sum()))                               # consumer on the default stream, immediately
        del clip
    torch.cuda.synchronize()
    for k, v in got:
        assert v.item() == want[k].item(), (k, v.item(), want[k].item())


def test_refusals():
    from maed_amd import data as D
    from maed_amd._lib import MaedHipError
    frames, records = R.random_scene(4, 1, 2, 16, 16, lo=40, hi=100, jitter=False)
    packed = D.pack_clips(frames, records, D.ClipAugment(16, 16))
    with pytest.raises(MaedHipError):                       # a CPU tensor is an error, never a fallback
        D.preprocess_clips(packed, out=torch.empty(1, 2, 3, 16, 16))
    with pytest.raises(NotImplementedError):
        D.ClipAugment(erase_fill=True)
    import dataclasses
    with pytest.raises(MaedHipError, match="too short for the tables"):       # a parameter array of the wrong length: the buffer ends inside the clip_f table
        D.preprocess_clips(dataclasses.replace(packed, blob=packed.blob[:packed.offsets[3] + 8].clone()))
