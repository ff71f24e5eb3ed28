"""Host geometry of the reference stitch (s2v_amd.stitch) against tests/golden/stitch_goldens.npz, recorded
from the reference's futils/alignment_stit.py by tests/golden/make_stitch_golden.py.

Bars:
* compute_transform, quads and crop boxes: EXACTLY the goldens (float64 sums and products in the same order);
  the QUAD coefficients likewise (Image.__transformer's order of operations);
* calc_alignment_coefficients: the four corner pixel centres of the output grid, mapped with our coefficients
  and with the golden ones, differ by <= 1e-6 px.  The reference's own formula (inv(a^T a) a^T b) misses an
  exact rational solve by up to 8.9e-9 px on rotated squares, so the bar is about 100 x the formula's own
  error; a wrong formula is off by whole pixels.  a6, a7 of a rotated square are rounding noise (~1e-12):
  coefficients are compared by where they map points, never value by value;
* smoothing: within 1e-9 px of the golden computed with scipy (float64 sums of <= 13 terms of magnitude < 1e3:
  an order-of-summation difference is ~13 * 2^-53 * 1e3 ~ 1e-12).
"""
import numpy as np
import pytest

import s2v_import  # noqa: F401
import stitch_cases as SC
from s2v_amd import stitch as ST


@pytest.fixture(scope="module")
def G(golden):
    return golden("stitch_goldens")


def _map(a, pts):
    pts = np.asarray(pts, dtype=np.float64)
    den = a[6] * pts[:, 0] + a[7] * pts[:, 1] + 1
    return np.stack([(a[0] * pts[:, 0] + a[1] * pts[:, 1] + a[2]) / den,
                     (a[3] * pts[:, 0] + a[4] * pts[:, 1] + a[5]) / den], 1)


@pytest.mark.parametrize("name", list(SC.LANDMARKS))
def test_compute_transform_exact(G, name):
    c, x, y = ST.compute_transform(SC.LANDMARKS[name], scale=1.0)
    assert np.array_equal(np.stack([c, x, y]), G[f"lm.{name}.cxy"])


@pytest.mark.parametrize("name", list(SC.QUAD_CASES))
def test_crop_box_and_quad_coefficients_exact(G, name):
    W, H, S, quad = SC.QUAD_CASES[name]
    before = quad.copy()
    table, boxes = ST.quad_table([quad], S, W, H)
    assert np.array_equal(quad, before)                                 # the caller's quad is not modified
    assert tuple(boxes[0]) == tuple(int(v) for v in G[f"quad.{name}.box"])
    assert np.array_equal(table[0, :8], G[f"quad.{name}.coef"])
    b = boxes[0]
    assert tuple(table[0, 8:]) == (b[0], b[1], b[2] - b[0], b[3] - b[1])


def test_quads_from_landmarks_exact(G):
    """landmarks -> compute_transform -> make_quads to the bit, on the Stitcher case: float32 points as a FAN
    detector returns them, the frame without a face reusing its predecessor's (as the generator builds them)."""
    lms, prev = [], None
    for lm in SC.STITCH_LMS:
        prev = prev if lm is None else np.asarray(lm, dtype=np.float32)
        lms.append(prev)
    quads = ST.face_quads(lms, scale=1.0)
    assert np.array_equal(np.stack(quads), G["stitcher.quads"])
    assert np.array_equal(quads[0], quads[1]) and not np.array_equal(quads[1], quads[2])
    cs, xs, ys = (np.stack(v) for v in zip(*(ST.compute_transform(lm) for lm in lms)))
    assert np.array_equal(ST.make_quads(cs, xs, ys), G["stitcher.quads"])


def test_crop_box_offsets_are_what_the_cases_claim(G):
    assert tuple(G["quad.topleft.box"][:2]) == (0, 0)                   # clipped at 0: no offset
    assert tuple(G["quad.botright.box"][2:]) == (48, 40)                # clipped at the frame's far edges
    assert min(G["quad.deep256.box"][:2]) > 0                           # a real offset
    assert tuple(G["quad.wide256.box"]) == (0, 0, 256, 256)             # no crop at all
    q = SC.QUAD_CASES["wide256"][3]
    qsize = np.hypot(*((q[3] - q[1]) / 2)) * 2
    assert int(np.floor(qsize / 256 * 0.5)) == 1                        # just under the shrink threshold


@pytest.mark.parametrize("name", list(SC.QUAD_CASES) + list(SC.PASTE_CASES))
def test_alignment_coefficients_map_the_corners(G, name):
    if name in SC.QUAD_CASES:
        W, H, S, quad = SC.QUAD_CASES[name]
        pa = quad + 0.5
    else:
        W, H, S, _, pa = SC.PASTE_CASES[name]
    mine = ST.calc_alignment_coefficients(pa, ST.square(S))
    gold = G[f"paste.{name}.coef"]
    corners = [[0.5, 0.5], [W - 0.5, 0.5], [0.5, H - 0.5], [W - 0.5, H - 0.5]]     # pixel centres of the output grid
    d = np.abs(_map(mine, corners) - _map(gold, corners)).max()
    print(f"{name}: corner centres move by {d:.3e} px")
    assert d <= 1e-6
    # and they are the right coefficients: pa lands on the square
    assert np.abs(_map(mine, pa) - np.array(ST.square(S), dtype=np.float64)).max() <= 1e-6


def test_trapezoid_is_a_true_perspective(G):
    assert np.abs(G["paste.trapezoid.coef"][6:]).min() > 1e-3
    assert np.abs(G["paste.inside.coef"][6:]).max() < 1e-9


def test_smoothing_matches_scipy_golden(G):
    cs, xs, ys = zip(*(ST.compute_transform(lm, scale=1.0) for lm in SC.SMOOTH_LMS))
    cs = ST.gaussian_filter1d(np.stack(cs), SC.SMOOTH_SIGMAS[0])
    xs = ST.gaussian_filter1d(np.stack(xs), SC.SMOOTH_SIGMAS[1])
    ys = ST.gaussian_filter1d(np.stack(ys), SC.SMOOTH_SIGMAS[1])
    quads = ST.make_quads(cs, xs, ys)
    d = np.abs(quads - G["smooth.quads"]).max()
    print(f"smoothed quads: max |d| {d:.3e} px")
    assert d <= 1e-9
    raw = ST.make_quads(*(np.stack(v) for v in zip(*(ST.compute_transform(lm) for lm in SC.SMOOTH_LMS))))
    assert np.abs(raw - G["smooth.quads"]).max() > 0.1                  # the smoothing moves the corners


def test_gaussian_filter_reflects_more_than_once_and_keeps_dtype():
    a = np.array([[1.0], [4.0], [2.0]])                                 # radius 6 on 3 samples: repeated reflection
    got = ST.gaussian_filter1d(a, 1.5)
    t = np.arange(-6, 7)
    k = np.exp(-0.5 / 2.25 * t ** 2)
    k /= k.sum()
    ext = np.array([a[(i % 6) if (i % 6) < 3 else 5 - (i % 6), 0] for i in range(-6, 9)])   # d c b a | a b c d
    ref = np.array([np.dot(k, ext[i:i + 13]) for i in range(3)])
    assert np.abs(got[:, 0] - ref).max() <= 1e-12
    assert ST.gaussian_filter1d(a.astype(np.float32), 1.5).dtype == np.float32


def test_raising_cases():
    W, H, S, quad = SC.SHRINK_QUAD
    with pytest.raises(ValueError, match="frame 0.*shrink"):
        ST.quad_table([quad], S, W, H)
    with np.errstate(invalid="ignore"):
        c, x, y = ST.compute_transform(-1.0 * np.ones([68, 2]))         # a frame without a face: 0 / 0
    nan_quad = ST.make_quads(c[None], x[None], y[None])[0]
    assert not np.isfinite(nan_quad).all()
    with pytest.raises(ValueError, match="frame 3.*non-finite"):
        ST.quad_table([SC.QUAD_CASES["inside"][3]] * 3 + [nan_quad], 32, 48, 40)
    with pytest.raises(ValueError, match="outside"):
        ST.crop_box(SC.PASTE_CASES["miss"][4], 32, 48, 40)
    with pytest.raises(NotImplementedError):
        ST.crop_image(None, 32, SC.QUAD_CASES["inside"][3], enable_padding=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ST.crop_image(np.zeros((40, 48, 3), np.uint8), 32, SC.QUAD_CASES["inside"][3])


def test_quad_coefficient_builder_against_pillow():
    Image = pytest.importorskip("PIL.Image")
    W, H, S, quad = SC.QUAD_CASES["botright"]
    frame = SC.image("botright", H, W)
    table, boxes = ST.quad_table([quad], S, W, H)
    l, t, r, b = boxes[0]
    rel = quad - [l, t]
    ref = np.array(Image.fromarray(frame[t:b, l:r]).transform((S, S), Image.QUAD, (rel + 0.5).flatten(),
                                                              Image.BILINEAR))
    got = SC.pil_quad(frame[t:b, l:r], table[0, :8], S)
    assert np.array_equal(got, ref)
    assert (ref.sum(2) == 0).mean() > 0.2 and (ref.sum(2) > 0).mean() > 0.2          # fill and samples both present


def test_numpy_restatement_reproduces_pillow_on_random_transforms():
    """The rules csrc/stitch.hip restates (bounds test before the half-pixel shift, clamped neighbours, truncation,
    the premultiplied RGBA round trip, BLEND8), as tests/stitch_cases.py states them in NumPy, against Pillow itself
    on random QUAD and PERSPECTIVE transforms of noise images: bit-exact."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    for it in range(60):
        h, w = (int(v) for v in rng.integers(5, 40, 2))
        S = int(rng.integers(4, 33))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        quad = SC.rotated_square(*rng.uniform(-5, [w + 5, h + 5]), rng.uniform(2, 30), rng.uniform(0, 360))
        if it % 5 == 0:
            quad = np.rint(quad) - 0.5                                   # samples on exact pixel centres
        ref = np.array(Image.fromarray(img).transform((S, S), Image.QUAD, (quad + 0.5).flatten(), Image.BILINEAR))
        assert np.array_equal(SC.pil_quad(img, ST.quad_coefficients(quad, S, S), S), ref), it
        ch = 3 + it % 2
        crop = rng.integers(0, 256, (S, S, ch), dtype=np.uint8)
        a = rng.uniform(-1, 1, 8) * [2, 1, S, 1, 2, S, 0.02, 0.02]
        pasted = Image.fromarray(img).convert("RGBA")
        proj = Image.fromarray(crop, "RGBA" if ch == 4 else "RGB").convert("RGBA").transform(
            (w, h), Image.PERSPECTIVE, a, Image.BILINEAR)
        pasted.paste(proj, (0, 0), mask=proj)
        assert np.array_equal(SC.pil_paste(crop, a, img), np.array(pasted.convert("RGB"))), (it, ch)
