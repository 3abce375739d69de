"""GPU: tn_otsu_thresholds through the C-ABI — histograms equal np.bincount exactly, thresholds equal the float64 restatement of
the declared recurrence exactly, and (independent of that recurrence) sit on the maximum of the brute-force between-class
variance; calculate_threshold on a dataset tree."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import otsu_reference as R
from thermo_nerf_amd import _hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 2, 15, 16, 17, 255, 4097, 307_200, 1_000_003)
CONTENTS = ("constant", "two_valued", "uniform", "bimodal")


def make_image(kind: str, n: int, rng) -> np.ndarray:
    if kind == "constant":  # one bin takes everything
        return np.full(n, int(rng.integers(0, 256)), dtype=np.uint8)
    if kind == "two_valued":  # a flat background with runs of a second value
        lo, hi = sorted(int(v) for v in rng.choice(256, 2, replace=False))
        out = np.full(n, lo, dtype=np.uint8)
        out[rng.random(n) < 0.3] = hi
        return out
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "bimodal":
        fg = rng.random(n) < 0.35
        v = np.where(fg, rng.normal(190.0, 14.0, n), rng.normal(60.0, 9.0, n))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    raise ValueError(kind)


def plateau_images(rng):
    """two to four distinct values with wide empty gaps: sigma is mathematically constant between neighbouring values"""
    cases = [((10, 200), (0.3, 0.7)), ((0, 255), (0.5, 0.5)), ((0, 255), (0.999, 0.001)), ((5, 100, 250), (0.2, 0.5, 0.3)),
             ((3, 90, 91, 240), (0.25, 0.25, 0.25, 0.25)), ((40, 41), (0.6, 0.4)), ((7, 128, 249), (1 / 3, 1 / 3, 1 / 3)),
             ((1, 64, 192, 254), (0.1, 0.4, 0.4, 0.1))]
    out = []
    for values, probs in cases:
        for n in (97, 5003, 70_001):
            out.append(rng.choice(np.array(values, dtype=np.uint8), size=n, p=np.array(probs) / np.sum(probs)))
    return out


def run(images, shift: int = 0, scratch=None):
    """one tn_otsu_thresholds call on the images packed back to back, the first one `shift` bytes behind an aligned address
    -> (histograms uint32 [N,256] as int64, thresholds [N], the 16-byte alignments the images started at, scratch)"""
    n = len(images)
    packed = np.concatenate([np.zeros(shift, dtype=np.uint8)] + [np.asarray(im, dtype=np.uint8).reshape(-1) for im in images])
    dev = torch.from_numpy(packed).to(DEV)
    offsets = (ctypes.c_int64 * (n + 1))()
    offsets[0] = shift
    for i, im in enumerate(images):
        offsets[i + 1] = offsets[i] + int(np.asarray(im).size)
    if scratch is None:
        scratch = torch.full((n, 256), -1, dtype=torch.int32, device=DEV)  # garbage: the call clears it itself
    thresholds = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    code = _hip.load().tn_otsu_thresholds(dev.data_ptr(), offsets, n, scratch.data_ptr(), thresholds.data_ptr(), _hip.current_stream())
    assert code == 0, code
    torch.cuda.synchronize()
    hist = scratch.cpu().numpy().view(np.uint32).astype(np.int64)
    starts = {(dev.data_ptr() + offsets[i]) % 16 for i in range(n)}
    return hist, thresholds.cpu().numpy(), starts, scratch


def check(images, hist, thresholds):
    for k, im in enumerate(images):
        flat = np.asarray(im, dtype=np.uint8).reshape(-1)
        assert flat.size <= 1 << 23  # the restatement itself meets the definition check's condition
        want = np.bincount(flat, minlength=256)
        assert np.array_equal(hist[k], want), (k, flat.size)
        restated = R.otsu_restated(want)
        print(f"image {k}: {flat.size} px, device threshold {int(thresholds[k])}, restated {restated}")
        assert int(thresholds[k]) == restated, (k, flat.size)
        # the definition, independent of the recalled recurrence: compare sigma, not the index (plateaus)
        assert R.smallest_class_fraction(want) >= 2.0 ** -23
        sigma = R.between_class_variance(want)
        assert sigma[int(thresholds[k])] >= (1.0 - 1e-12) * sigma.max(), (k, flat.size)


@pytest.mark.parametrize("kind", CONTENTS)
def test_single_images_of_every_size_and_content(kind):
    rng = np.random.default_rng(CONTENTS.index(kind) + 11)
    for j, n in enumerate(SIZES):
        image = make_image(kind, n, rng)
        hist, thr, _, scratch = run([image], shift=(5 * j + 3) % 16)
        check([image], hist, thr)
        if kind == "constant":
            assert int(thr[0]) == 0
        # the same scratch again: the call does its own clearing
        hist2, thr2, _, _ = run([image], shift=(5 * j + 3) % 16, scratch=scratch)
        assert np.array_equal(hist2, hist) and np.array_equal(thr2, thr)


def test_mixed_images_in_one_call_start_at_every_alignment():
    rng = np.random.default_rng(5)
    seen = set()
    for n_images in range(1, 41):
        images = []
        for j in range(n_images):
            size = 1 + 2 * int(rng.integers(0, 400)) if j % 7 else int(rng.choice(SIZES[:7]))  # mixed odd sizes (+ the small fixed ones)
            images.append(make_image(CONTENTS[(j + n_images) % 4], size, rng))
        hist, thr, starts, scratch = run(images, shift=n_images % 16)
        seen |= starts
        check(images, hist, thr)
        if n_images in (1, 17, 40):
            hist2, thr2, _, _ = run(images, shift=n_images % 16, scratch=scratch)
            assert np.array_equal(hist2, hist) and np.array_equal(thr2, thr)
    assert seen == set(range(16))


def test_every_size_and_content_in_one_call():
    rng = np.random.default_rng(17)
    images = [make_image(kind, n, rng) for n in SIZES for kind in CONTENTS]
    hist, thr, _, _ = run(images, shift=9)
    check(images, hist, thr)


def test_more_images_than_one_launch_carries():
    """the histogram pass takes its image extents by value, 128 images per launch: 300 images cross two batch boundaries"""
    rng = np.random.default_rng(23)
    images = [make_image(CONTENTS[j % 4], 33 + 2 * int(rng.integers(0, 300)), rng) for j in range(300)]
    hist, thr, _, _ = run(images, shift=1)
    check(images, hist, thr)


def test_plateaus_and_the_fixture_image(golden_dir):
    rng = np.random.default_rng(29)
    images = plateau_images(rng)
    fixture = np.asarray(Image.open(os.path.join(golden_dir, "thermal", "IMG_3561.PNG")), dtype=np.uint8)
    images.append(fixture)
    hist, thr, _, _ = run(images, shift=7)
    check(images, hist, thr)
    assert int(thr[-1]) == 53


def test_python_surface_matches_the_c_abi():
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import otsu_thresholds

    rng = np.random.default_rng(31)
    images = [make_image("bimodal", 24 * 31, rng).reshape(24, 31), make_image("uniform", 7, rng),
              make_image("two_valued", 3 * 5 * 5, rng).reshape(3, 5, 5)]
    thr, hist = otsu_thresholds([torch.from_numpy(im).to(DEV) for im in images], return_histograms=True)
    assert thr.dtype == torch.int32 and thr.shape == (3,) and thr.is_cuda and hist.shape == (3, 256)
    check(images, hist.cpu().numpy().astype(np.int64), thr.cpu().numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        otsu_thresholds([torch.from_numpy(images[0])])
    with pytest.raises(TypeError):
        otsu_thresholds([torch.zeros(4, 4, device=DEV)])  # float pixels


def test_calculate_threshold_on_a_dataset_tree(tmp_path):
    """a transforms.json tree with train and eval frames (as tests/test_gpu_training.py builds it): every frame counts, and the
    result is sum(restated thresholds) / N / 255.0 as a Python float, exactly"""
    from thermo_nerf_amd import ModelType, synthetic
    from thermo_nerf_amd.thermal_nerf.calculate_threshold import calculate_threshold

    res, n = 32, 10
    cams = synthetic.orbit_cameras(res, res, list(range(n)), num_views=n, elevation_deg=[(0.0, 25.0)[v % 2] for v in range(n)])
    (tmp_path / "images").mkdir()
    (tmp_path / "thermal").mkdir()
    frames, greys, rgb_greys = [], [], []
    for i in range(n):
        rb = cams.generate_rays(i, device=DEV)
        rgb, th = synthetic.analytic_scene(rb.origins, rb.directions)
        name = f"frame_{'eval' if i % 5 == 4 else 'train'}_{i:04d}.png"
        rgb8 = (rgb.cpu().numpy() * 255).round().astype(np.uint8)
        th8 = (th[..., 0].cpu().numpy() * 255).round().astype(np.uint8)
        Image.fromarray(rgb8).save(tmp_path / "images" / name)
        Image.fromarray(th8, mode="L").save(tmp_path / "thermal" / name)
        greys.append(th8)
        rgb_greys.append(np.asarray(Image.fromarray(rgb8).convert("L")))
        c2w = torch.cat([cams.camera_to_worlds[i], torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
        frames.append({"file_path": f"images/{name}", "thermal_file_path": f"thermal/{name}", "transform_matrix": c2w})
    f = float(cams.fx[0])
    (tmp_path / "transforms.json").write_text(json.dumps(
        {"fl_x": f, "fl_y": f, "cx": res / 2, "cy": res / 2, "w": res, "h": res, "frames": frames}))

    def restated(images):
        ts = [R.otsu_restated(np.bincount(im.reshape(-1), minlength=256)) for im in images]
        return sum(ts) / len(ts) / 255.0

    got = calculate_threshold(tmp_path, ModelType.THERMONERF, device=DEV)
    print("calculate_threshold", got, "restated", restated(greys))
    assert isinstance(got, float) and got == restated(greys)
    assert 0.0 < got < 1.0
    assert calculate_threshold(tmp_path / "transforms.json", device=DEV) == got
    assert calculate_threshold(tmp_path, ModelType.NERFACTO, device=DEV) == restated(rgb_greys)  # the file_path images
