"""The conditions that tests/test_iou3d_gpu.py and test_post_process_gpu.py rely on, proved for the references alone on
the CPU: the exact clipper and the oracle reproduce the hand-derived areas, the exact-area scenes have few pairs in
inside_box's margin band, every exact NMS scene has no pair IoU near its threshold, chain_scene's keep list is what
the oracle keeps, and few points of the point scenes lie near a face.  Run with -s to see every figure."""
import numpy as np
import pytest

import box_geometry_cases as bg
import test_iou3d_gpu as cases


def test_clipper_reproduces_the_table():
    for name, a, b, area, kind in bg.CLOSED_FORM:
        if kind != 'exact':
            continue
        for x, y in ((a, b), (b, a)):
            got = bg.clip_area64(x, y)
            assert abs(got - area) <= 1e-12, (name, got, area)


def test_oracle_reproduces_the_table(oracle):
    a, b, area, kinds = bg.closed_form_arrays()
    worst = 0.0
    for x, y in ((a, b), (b, a)):
        full = oracle.boxes_overlap_bev(x, y).astype(np.float64)
        aligned = oracle.boxes_aligned_overlap_bev(x, y).astype(np.float64)
        assert np.isfinite(full).all()
        for r, row in enumerate(bg.CLOSED_FORM):
            print("%-44s area %.9g  oracle %.9g" % (row[0], area[r], full[r, r]))
            assert abs(full[r, r] - area[r]) <= cases.TABLE_TOL, row[0]
            assert aligned[r] == full[r, r], row[0]
            worst = max(worst, abs(full[r, r] - area[r]))
    print("oracle against the table: max error %.3e" % worst)


def test_margin_band_marks_the_quirk_rows_only_where_it_should():
    """the band holds the pinned quirk and the touching rows, not the clean overlaps"""
    band = {row[0]: bool(bg.margin_band(row[1], row[2])) for row in bg.CLOSED_FORM if row[4] != 'nan'}
    assert band['quirk: gap of 0.005'] and band['shared edge'] and band['shared corner'] and band['gap of 0.02']
    assert band['half shift']                          # its corners lie on the other box's long edges
    assert not band['far apart'] and not band['cross 6 x 1, h=0.4']
    assert not band['nested, rotated'] and not band['slivers 10 x 0.05 at +-0.3']


@pytest.mark.parametrize("offset", cases.OFFSETS)
def test_exact_area_scenes(oracle, offset):
    a, b, exact, clear = cases.exact_scene_reference(offset)
    ref = oracle.boxes_overlap_bev(a, b).astype(np.float64)
    in_band = int((~clear).sum())
    err = float(np.abs(ref - exact)[clear].max())
    print("offset %s: %d of %d pairs in the margin band, %d overlap, max |oracle - exact| %.3e"
          % (offset, in_band, clear.size, int((exact > 0).sum()), err))
    assert clear.size == 3600 and in_band <= 0.02 * clear.size
    assert (exact > 0).sum() >= 500


@pytest.mark.parametrize("n,spread,nominal,normal", cases.NMS_EXACT)
def test_nms_scenes_have_a_clear_threshold(oracle, n, spread, nominal, normal):
    boxes, scores, order = cases.nms_scene(n, spread)
    thresh, half = bg.gap_threshold(cases.scene_iou(oracle, boxes[order], normal), nominal)
    kept = oracle.nms(boxes[order], thresh, normal=normal)
    print("n %d spread %g nominal %g normal %d: threshold %.7f, half-gap %.3e, kept %d"
          % (n, spread, nominal, normal, thresh, half, len(kept)))
    assert abs(thresh - nominal) <= 0.25 * nominal
    assert half >= cases.MIN_HALF_GAP
    assert 0 < len(kept) < n


def test_gap_threshold_and_greedy_keep_by_hand():
    iou = np.zeros((4, 4))
    iou[0, 1], iou[0, 2], iou[1, 3], iou[2, 3] = 0.26, 0.30, 0.36, 0.9
    t, half = bg.gap_threshold(iou, 0.3)               # values in [0.225, 0.375]: 0.26, 0.30, 0.36 -> widest gap 0.30 .. 0.36
    assert abs(t - 0.33) < 1e-7 and abs(half - 0.03) < 1e-7
    # 0 removes 1; 1, removed, does not remove 3; 2 removes 3
    sup = np.zeros((4, 4), bool)
    sup[0, 1] = sup[1, 3] = True
    assert bg.greedy_keep(sup).tolist() == [0, 2, 3]
    sup[2, 3] = True
    assert bg.greedy_keep(sup).tolist() == [0, 2]


def test_iou_normal_restated_decides_as_the_oracle(oracle):
    """iou_normal is + - * / max min in fp32: the numpy restatement and the oracle's C agree on every decision, so the
    large axis-aligned case needs no tie band"""
    n, thresh, normal = cases.NMS_LARGE[3]
    assert normal
    boxes, scores, order = cases.nms_scene(n, 12.0)
    iou = bg.iou_normal_np(boxes[order], boxes[order])
    assert np.array_equal(bg.greedy_keep(iou > np.float32(thresh)), oracle.nms(boxes[order], thresh, normal=True))
    assert np.array_equal(bg.hybrid_keep(iou, iou, thresh), bg.greedy_keep(iou > np.float32(thresh)))


def test_chain_scene_keep_list_is_the_oracles(oracle):
    n = 4200
    boxes, scores, order, keep = bg.chain_scene_of(n, seed=n)
    assert boxes.shape == (n, 7) and np.array_equal(order, np.argsort(-scores, kind="stable"))
    assert np.array_equal(order[oracle.nms(boxes[order], 0.3)], keep)
    assert len(keep) == 2 * (n // 3)


@pytest.mark.parametrize("n,b_last", [(200, False), (4097, False), (16384, False), (16384, True), (16385, True)])
def test_chain_scene_layout(oracle, n, b_last):
    """the properties the by-construction keep list rests on, on the oracle's own IoUs (a sample of sites at large n),
    and where the members of a site fall among nms_walk's blocks and slots"""
    boxes, scores, order, keep = bg.chain_scene_of(n, seed=n, b_last=b_last)
    ns = n // 3
    assert boxes.shape[0] == n and len(keep) == 2 * ns + (n % 3 > 0)
    rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    kept = np.zeros(n, bool); kept[keep] = True
    # every suppressed box has exactly the two partners of its site above the threshold, both kept and both near 0.4286
    sample = np.nonzero(~kept)[0][:: max(1, (n - len(keep)) // 150)]
    iou = oracle.boxes_iou_bev(boxes[sample], boxes)
    for row, s in zip(iou, sample):
        row = row.copy(); row[s] = 0
        over = np.nonzero(row > 0.3 - 0.12)[0]
        assert len(over) in (1, 2) and kept[over].all() and (np.abs(row[over] - 0.6 / 1.4) < 2e-3).all()
        assert (row[row <= 0.18] <= 0.154).all() and ((row == 0).sum() >= n - 3)
        assert (rank[over] >> 6 != rank[s] >> 6).all() or n < 3 * 64
        if n >= 12288:
            assert (rank[over] >> 12 != rank[s] >> 12).all()
        if not b_last:
            assert rank[over].min() < rank[s] and (len(over) == 1 or rank[over].max() > rank[s])
    slots = np.unique(rank[~kept] >> 12)
    print("n %d b_last %d: suppressed boxes in slots %s" % (n, b_last, slots.tolist()))
    if n >= 16384:
        assert slots.tolist() == ([2, 3] + ([4] if n > 16384 else []) if b_last else [1, 2])


def test_point_scenes_have_few_points_near_a_face():
    for (B, T, M), (pts, boxes) in cases.all_point_scenes():
        near = cases.near_face_mask(pts, boxes)
        print("B %d T %d M %d: %d of %d points within 1e-4 of a face (%.3f %%)" % (B, T, M, near.sum(), near.size, 100 * near.mean()))
        assert near.mean() <= 0.005


def test_near_face_by_hand():
    box = np.array([[0, 0, 0, 4, 2, 2, 0.0], [100, 0, 0, 4, 2, 2, 0.0]])
    pts = np.array([[2.00005, 0, 0],        # 5e-5 outside the x face
                    [1.9, 0.99995, 0],      # 5e-5 inside the y face
                    [0, 0, 1.00005],        # above the top
                    [1.0, 0.5, 0.5],        # well inside
                    [98.00005, 0, 5.0],     # at box 1's x face plane but far above it: that box cannot decide the point
                    [2.00005, 50.0, 0]])    # on box 0's x face plane, far outside its circle
    assert bg.near_face(pts, box).tolist() == [True, True, True, False, False, False]


def test_chunk_scene_expectations_are_the_oracles(oracle):
    for T, M in cases.CHUNK_CASES:
        pts, boxes, expected = cases.chunk_scene(T, M)
        ref = oracle.points_in_boxes(pts, boxes)[0]
        known = expected != -2
        assert known.sum() == min(T, M, 200) and np.array_equal(ref[known], expected[known])
        assert (ref == -1).any()
        if T > 130:
            both = np.nonzero(known)[0][-1]
            one = lambda k: oracle.points_in_boxes(pts[:, both:both + 1], boxes[:, k:k + 1])[0, 0]
            assert one(3) == 0 and one(130) == 0 and expected[both] == 3
