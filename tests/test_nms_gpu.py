"""s2v_nms (csrc/nms.hip) called directly through ctypes.

Bar: BIT-EXACT.  The kernel copies rows and decides with the reference's own fp32 expressions, unfused and
with a correctly rounded divide, so the kept position indices and every float of every kept row equal
face.py_cpu_nms on the position-sorted rows (distinct scores), and nms_cases.contract where the pre-filter,
top_k, keep_max, equal scores, NaN or the capacity come in.  ``out`` is filled with a sentinel first: rows
past min(kept, keep_max) of an image and the floats past the last image must still hold it."""
import math

import numpy as np
import pytest
import torch

import nms_cases as NC
import s2v_import  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = np.float32(-777.25)
PAD = 64                                                                   # floats past the last image's rows


def run(images, rs, thresh, min_score=-math.inf, top_k=0, keep_max=None, max_cand=None):
    """One s2v_nms launch over the images' rows (each [K, rs], slot order) -> per image (the whole out block
    [keep_max, rs], kept, status), after checking the floats past the last block."""
    from s2v_amd import _lib
    lib = _lib.load()
    n = len(images)
    max_cand = max_cand or max(1, max(len(r) for r in images))
    keep_max = keep_max or max_cand
    cand = np.full((n, max_cand, rs), 12345.0, np.float32)                 # rows past count: garbage that scores high
    for b, r in enumerate(images):
        cand[b, : len(r)] = r
    dc = torch.from_numpy(cand).to(DEV)
    dn = torch.tensor([len(r) for r in images], dtype=torch.int32, device=DEV)
    out = torch.full((n * keep_max * rs + PAD,), float(SENTINEL), device=DEV)
    kept = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    status = torch.full((n,), -5, dtype=torch.int32, device=DEV)
    _lib.check(lib.s2v_nms(dc.data_ptr(), dn.data_ptr(), n, max_cand, rs, thresh, min_score, top_k, keep_max,
                           out.data_ptr(), kept.data_ptr(), status.data_ptr(),
                           torch.cuda.current_stream().cuda_stream), "s2v_nms")
    ho = out.cpu().numpy()
    assert (ho[n * keep_max * rs:] == SENTINEL).all()
    ho = ho[: n * keep_max * rs].reshape(n, keep_max, rs)
    return [(ho[b], int(k), int(s)) for b, (k, s) in enumerate(zip(kept.cpu().tolist(), status.cpu().tolist()))]


def assert_rows(block, kept, status, exp_rows, exp_kept=None, exp_status=NC.OK):
    """The out block of one image: its first rows bit-equal to exp_rows, the rest untouched."""
    assert status == exp_status and kept == (len(exp_rows) if exp_kept is None else exp_kept)
    m = len(exp_rows)
    assert NC.position_index(block[:m]).tolist() == NC.position_index(exp_rows).tolist()
    assert np.array_equal(block[:m].view(np.uint32), exp_rows.view(np.uint32))
    assert (block[m:] == SENTINEL).all()


@pytest.mark.parametrize("rs", [8, 16])
@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 65, 257, 1000])
def test_nms_bit_equal_to_py_cpu_nms(k, rs):
    rows = NC.clustered(100 * k + rs, k, rs)
    for thresh in (0.3, 0.4):
        exp = NC.by_py_cpu_nms(rows, thresh)
        if k >= 63:
            assert 1 < len(exp) < k
        (block, kept, status), = run([rows], rs, thresh)
        assert_rows(block, kept, status, exp)


def test_nms_three_images_in_one_launch():
    imgs = [NC.clustered(1, 130, 8), NC.clustered(2, 0, 8), NC.clustered(3, 65, 8)]
    res = run(imgs, 8, 0.3, max_cand=200)
    for rows, (block, kept, status) in zip(imgs, res):
        assert_rows(block, kept, status, NC.by_py_cpu_nms(rows, 0.3))
    assert res[1][1] == 0 and res[0][1] > 1 and res[2][1] > 1


def test_nms_min_score_top_k_keep_max():
    rows = NC.clustered(9, 600, 16)
    full = NC.by_py_cpu_nms(rows, 0.4)
    # S3FD's pre-filter equals filtering after the NMS
    (block, kept, status), = run([rows], 16, 0.4, min_score=0.5)
    exp, _, _ = NC.contract(rows, 0.4, min_score=0.5)
    assert np.array_equal(exp, full[full[:, 5] > 0.5]) and 0 < len(exp) < len(full)
    assert_rows(block, kept, status, exp)
    # top_k below, at and above the row count
    for top_k in (1, 64, 100, 600, 5000):
        exp, n_exp, _ = NC.contract(rows, 0.4, top_k=top_k)
        (block, kept, status), = run([rows], 16, 0.4, top_k=top_k)
        assert_rows(block, kept, status, exp)
    assert len(NC.contract(rows, 0.4, top_k=100)[0]) < len(full)
    # keep_max below the kept count: the count is reported uncapped, only keep_max rows are written
    for keep_max in (1, 7, len(full) - 1, len(full), len(full) + 1):
        (block, kept, status), = run([rows], 16, 0.4, keep_max=keep_max)
        assert_rows(block, kept, status, full[:keep_max], exp_kept=len(full))
    # all three at once, two images
    imgs = [rows, NC.clustered(10, 300, 16)]
    res = run(imgs, 16, 0.3, min_score=0.2, top_k=90, keep_max=11)
    for r, (block, kept, status) in zip(imgs, res):
        exp, n_exp, _ = NC.contract(r, 0.3, min_score=0.2, top_k=90, keep_max=11)
        assert n_exp > 11
        assert_rows(block, kept, status, exp, exp_kept=n_exp)


def test_nms_overlap_equal_to_the_threshold_survives():
    # [0,0,9,9] (area 100) and [0,0,9,4] (area 50): inter 50, ovr = 50 / (100 + 50 - 50) = 0.5 exactly
    rows = NC.boxes([[0, 0, 9, 9], [0, 0, 9, 4]], [0.9, 0.8])
    (block, kept, status), = run([rows], 8, 0.5)
    assert_rows(block, kept, status, rows)
    # [0,0,9,5]: inter 60, ovr 0.6 > 0.5 is suppressed; [0,0,19,9] and [0,0,9,9]: ovr 100 / 200 at 0.5 survives
    rows = NC.boxes([[0, 0, 9, 9], [0, 0, 9, 5], [40, 0, 59, 9], [40, 0, 49, 9]], [0.9, 0.8, 0.7, 0.6])
    (block, kept, status), = run([rows], 8, 0.5)
    assert_rows(block, kept, status, rows[[0, 2, 3]])
    # areas 100 and 30, inter 30: ovr = fp32(30 / 100), which survives the fp32 threshold 0.3 and the next value
    # above it, and goes at the next value below
    rows = NC.boxes([[0, 0, 9, 9], [0, 0, 9, 2]], [0.9, 0.8])
    t = np.float32(0.3)
    for thr, n_exp in ((t, 2), (np.nextafter(t, np.float32(1)), 2), (np.nextafter(t, np.float32(0)), 1)):
        exp = NC.by_py_cpu_nms(rows, thr)
        assert len(exp) == n_exp
        (block, kept, status), = run([rows], 8, float(thr))
        assert_rows(block, kept, status, exp)


def test_nms_zero_area_pair_suppresses_through_nan():
    rows = NC.boxes([[5, 5, 4, 4], [5, 5, 4, 4], [50, 50, 60, 60]], [0.9, 0.8, 0.7])
    (block, kept, status), = run([rows], 8, 0.3)
    assert_rows(block, kept, status, rows[[0, 2]])                         # 0 / 0: the second box goes
    assert len(NC.contract(rows, 0.3)[0]) == 2


def test_nms_equal_scores_take_the_larger_position_index_first():
    rows = NC.disjoint([0.5, 0.9, 0.5, 0.9, 0.5])[[4, 0, 3, 1, 2]]         # position indices 3 5 7 9 11, shuffled
    (block, kept, status), = run([rows], 8, 0.3)
    assert NC.position_index(block[:5]).tolist() == [9, 5, 11, 7, 3]
    for seed, k in ((21, 64), (22, 500), (23, 1000)):
        rows = NC.with_ties(seed, k, 16)
        exp, _, _ = NC.contract(rows, 0.3)
        (block, kept, status), = run([rows], 16, 0.3)
        assert_rows(block, kept, status, exp)
        # the same rows in another slot order give the same answer
        (block, kept, status), = run([rows[::-1].copy()], 16, 0.3)
        assert_rows(block, kept, status, exp)


def test_nms_orders_any_finite_score():
    tiny = np.float32(1e-45)
    scores = [3.0e38, -3.0e38, 0.0, -0.0, tiny, -tiny, 1.0, np.nextafter(np.float32(1), np.float32(0)), -1.0, 0.5,
              np.float32(np.inf), 1.17549435e-38]
    rows = NC.disjoint(scores)
    exp, n_exp, _ = NC.contract(rows, 0.3)
    assert n_exp == len(scores)                                            # min_score -inf drops nothing finite
    (block, kept, status), = run([rows[::-1].copy()], 8, 0.3)
    assert_rows(block, kept, status, exp)
    exp, n_exp, _ = NC.contract(rows, 0.3, min_score=0.0)                  # !(score > 0): zeros and negatives go
    (block, kept, status), = run([rows], 8, 0.3, min_score=0.0)
    assert n_exp == 7
    assert_rows(block, kept, status, exp)


def test_nms_nan_score_and_capacity():
    from s2v_amd import _lib
    cap = _lib.load().s2v_nms_capacity()
    assert cap >= 5000
    ok = NC.clustered(5, 40, 8)
    bad = ok.copy()
    bad[17, 5] = np.nan
    res = run([ok, bad, ok], 8, 0.3, min_score=0.5)
    exp, _, _ = NC.contract(ok, 0.3, min_score=0.5)
    assert_rows(*res[0], exp)
    assert_rows(*res[1], ok[:0], exp_status=NC.NAN_SCORE)                 # status 2, kept 0, nothing written
    assert_rows(*res[2], exp)
    # capacity + 1 rows: status 1 and out untouched; the image beside it is served
    over = NC.clustered(6, cap + 1, 8, extent=3000.0)
    res = run([over, ok], 8, 0.3, keep_max=64)
    assert_rows(*res[0], ok[:0], exp_status=NC.OVER_CAPACITY)
    assert_rows(res[1][0], res[1][1], res[1][2], NC.by_py_cpu_nms(ok, 0.3)[:64], exp_kept=len(NC.by_py_cpu_nms(ok, 0.3)))
    # the pre-filter counts first: the same rows pass with fewer than capacity above min_score
    exp, n_exp, st = NC.contract(over, 0.3, min_score=0.5, capacity=cap)
    assert st == NC.OK and n_exp > 64
    (block, kept, status), = run([over], 8, 0.3, min_score=0.5, keep_max=n_exp)
    assert_rows(block, kept, status, exp)


def test_nms_top_k_cuts_an_image_above_capacity():
    """More rows than the sort holds pass step 1, but step 3 leaves top_k <= capacity of them: the kernel takes
    the first top_k by key (RetinaFace's 5000; the capacity itself; 1) and answers as the contract does; top_k
    above the capacity is status 1."""
    from s2v_amd import _lib
    cap = _lib.load().s2v_nms_capacity()
    rows = NC.clustered(11, cap + 3000, 16, extent=4000.0)
    tied = NC.with_ties(12, cap + 700, 8, levels=50)                       # the top_k-th score is shared by many rows
    for imgs, rs in (([rows], 16), ([tied, NC.clustered(13, 70, 8)], 8)):
        for top_k, min_score in ((5000, -math.inf), (cap, 0.06), (1, -math.inf)):
            res = run(imgs, rs, 0.4, min_score=min_score, top_k=top_k, keep_max=2048)
            for r, (block, kept, status) in zip(imgs, res):
                exp, n_exp, st = NC.contract(r, 0.4, min_score=min_score, top_k=top_k, keep_max=2048, capacity=cap)
                assert st == NC.OK and n_exp >= 1
                assert_rows(block, kept, status, exp, exp_kept=n_exp)
    (block, kept, status), = run([rows], 16, 0.4, top_k=cap + 1, keep_max=16)
    assert_rows(block, kept, status, rows[:0], exp_status=NC.OVER_CAPACITY)


def test_nms_full_capacity_and_slots_past_65535():
    from s2v_amd import _lib
    cap = _lib.load().s2v_nms_capacity()
    rows = NC.clustered(7, cap, 8, extent=3000.0)                          # exactly capacity rows: the whole sort
    exp, n_exp, _ = NC.contract(rows, 0.3)
    (block, kept, status), = run([rows], 8, 0.3, keep_max=n_exp + 3)
    assert_rows(block, kept, status, exp)
    # 70 000 rows of which 500 pass min_score, the passing ones in the highest slots
    k = 70000
    many = NC.clustered(8, k, 8, extent=3000.0)
    many = many[np.argsort(many[:, 5], kind="stable")]                     # slot order: score ascending
    floor = float(many[k - 501, 5])
    exp, n_exp, _ = NC.contract(many, 0.3, min_score=floor)
    assert (many[k - 500:, 5] > floor).all() and 1 < n_exp < 500
    (block, kept, status), = run([many], 8, 0.3, min_score=floor, keep_max=512)
    assert_rows(block, kept, status, exp)
