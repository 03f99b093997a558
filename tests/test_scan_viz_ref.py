"""CPU: the NumPy restatement of the scan pictures (tests/scan_viz_ref.py) held to facts worked by hand from the
definitions in include/tdr.h, "the scan picture" (reference: src/top_down_render.cpp:266-305)."""
from fractions import Fraction

import numpy as np
import scan_viz_ref as S

F32 = np.float32
NAN, INF = np.nan, np.inf
UNFLATTEN = [10, 20, 30]
LUT = np.stack([np.arange(256), 255 - np.arange(256), np.arange(256) ^ 0x5A], axis=1).astype(np.uint8)


def colour(label):
    return [label, 255 - label, label ^ 0x5A]


def test_2x3_render_of_three_classes_by_hand():
    rows, cols = 2, 3
    # per Eigen element (i, j) the three class values; linear index p = i + j * rows
    cells = {
        (0, 0): (1, 5, 2),          # class 1 wins                                   -> 20
        (1, 0): (7, 3, 7),          # classes 0 and 2 tie: the LAST one              -> 30
        (0, 1): (4, 4, 4),          # all equal, non-zero                            -> 255
        (1, 1): (0, 0, 0),          # all zero                                       -> 255
        (0, 2): (3, NAN, 1),        # the NaN takes part in nothing: class 0 wins    -> 10
        (1, 2): (NAN, NAN, NAN),    # every value NaN: best_cls stays 255            -> 255
    }
    want_label = {(0, 0): 20, (1, 0): 30, (0, 1): 255, (1, 1): 255, (0, 2): 10, (1, 2): 255}
    imgs = np.zeros((3, rows * cols), F32)
    for (i, j), v in cells.items():
        imgs[:, i + j * rows] = v
    pic = S.scan_picture(imgs, rows, cols, UNFLATTEN, LUT)
    assert pic.shape == (cols, rows, 3) and pic.dtype == np.uint8          # height = cols, width = rows
    for (i, j), lab in want_label.items():
        assert pic[j, i].tolist() == colour(lab), (i, j)                      # Eigen (i, j) lands at pixel y = j, x = i
    assert pic[0, 1].tolist() == colour(30)                                   # Eigen (1, 0) -> y = 0, x = 1, spelled out
    # the whole image, written out
    assert pic.tolist() == [[colour(20), colour(30)], [colour(255), colour(255)], [colour(10), colour(255)]]


def test_nan_in_the_winning_position_is_ignored():
    # class 2 would win the >= chain by position; being NaN it changes nothing and class 1 keeps the maximum
    assert S.labels(np.asarray([[1], [6], [NAN]], F32), UNFLATTEN).tolist() == [20]
    assert S.labels(np.asarray([[NAN], [6], [1]], F32), UNFLATTEN).tolist() == [20]


def test_exactly_one_non_nan_class_is_unknown():
    # best = worst = the one value
    assert S.labels(np.asarray([[NAN], [3], [NAN]], F32), UNFLATTEN).tolist() == [255]
    assert S.labels(np.asarray([[-2], [NAN], [NAN]], F32), UNFLATTEN).tolist() == [255]


def test_one_class_is_unknown_everywhere():
    imgs = np.asarray([[0, 1, 5, -3, NAN, INF]], F32)
    assert S.labels(imgs, [7]).tolist() == [255] * 6
    assert (S.scan_picture(imgs, 2, 3, [7], LUT) == np.asarray(colour(255), np.uint8)).all()


def test_infinities():
    cases = [((-INF, 3, INF), 30),        # +inf is the maximum
             ((INF, INF, 1), 20),         # two +inf: the last of them
             ((-INF, -INF, 2), 30),       # -inf >= -inf moves best_cls along; 2 wins
             ((2, -INF, -INF), 10),
             ((-INF, -INF, -INF), 255),   # best = worst = -inf
             ((INF, INF, INF), 255),      # worst stays +inf (inf < inf is false), best = +inf
             ((INF, NAN, -INF), 10)]
    imgs = np.asarray([c for c, _ in cases], F32).T
    assert S.labels(imgs, UNFLATTEN).tolist() == [w for _, w in cases]


def test_unflatten_is_stored_into_a_byte():
    assert S.labels(np.asarray([[1], [0]], F32), [256 + 17, 3]).tolist() == [17]
    assert S.labels(np.asarray([[1], [0]], F32), [-1, 3]).tolist() == [255]


# ---- analog ----------------------------------------------------------------------------------------------------------------
A50 = Fraction(10695475, 2097152)      # (float)(255.0 / 50.0) = 0x1.466666p+2 = 5.099999904632568359375


def test_scale_50_multiplier_is_the_float32_one():
    assert Fraction(float(F32(255.0 / 50.0))) == A50


def test_analog_scale_50_by_hand():
    # exact products v * a (v the float32 nearest the decimal) and their lrintf:
    #   0      -> 0
    #   0.098  -> 0.49979997...  -> 0
    #   0.1    -> 0.50999999...  -> 1
    #   0.294  -> 1.49939997...  -> 1
    #   0.3    -> 1.53000003...  -> 2
    #   50     -> 254.999995...  -> 255 (the float32 product is 255.0 or just below: 255 either way)
    #   51     -> 260.0999...    -> 255 (clamped)
    assert S.grey([0, 0.098, 0.1, 0.294, 0.3, 50, 51], 50).tolist() == [0, 0, 1, 1, 2, 255, 255]
    assert S.grey([-1, NAN, INF, -INF], 50).tolist() == [0, 0, 0, 0]
    assert S.grey([-1, NAN, INF, -INF, 1e30, -1e30], 1).tolist() == [0] * 6


def test_analog_float32_product_on_a_half_rounds_to_even():
    # float32 values whose EXACT product with a is not a half but whose float32 product is: lrintf sees the half
    halves = [(float.fromhex("0x1.919192p-4"), Fraction(1, 2), 0),     # exact 0.49999999885 -> 0.5 -> 0
              (float.fromhex("0x1.2d2d2ep-2"), Fraction(3, 2), 2),     # exact 1.50000003    -> 1.5 -> 2
              (float.fromhex("0x1.f5f5f6p-2"), Fraction(5, 2), 2),     # exact 2.49999996    -> 2.5 -> 2
              (float.fromhex("0x1.f5f5f8p-2"), Fraction(5, 2), 2),     # exact 2.50000011    -> 2.5 -> 2 (a double product would give 3)
              (float.fromhex("0x1.5f5f60p-1"), Fraction(7, 2), 4)]     # exact 3.50000003    -> 3.5 -> 4
    for v, half, want in halves:
        assert float(F32(v)) == v                                              # a float32 value
        exact = Fraction(v) * A50
        ulp = Fraction(1, 2 ** 25) if half < 1 else Fraction(1, 2 ** 23) if half < 2 else Fraction(1, 2 ** 22)   # float32 spacing just below the half
        assert exact != half and abs(exact - half) < ulp / 2                   # so the float32 product is the half
        assert S.grey([v], 50).tolist() == [want], v
    # and with a = 1 (scale 255) the halves themselves
    assert S.grey([0.5, 1.5, 2.5, 3.5, 254.5, 255.5], 255).tolist() == [0, 2, 2, 4, 254, 255]


def test_analog_picture_orientation():
    rows, cols = 2, 3
    img = np.zeros(rows * cols, F32)
    img[1 + 0 * rows] = 1.0                                                    # Eigen (1, 0)
    pic = S.analog_picture(img, rows, cols, 1.0)
    assert pic.shape == (cols, rows, 3)
    assert pic[0, 1].tolist() == [255, 255, 255] and int(pic.astype(int).sum()) == 3 * 255


def test_label_picture():
    lab = np.asarray([[0, 255], [7, 7], [128, 1]], np.uint8)
    assert S.label_picture(lab, LUT).tolist() == [[colour(0), colour(255)], [colour(7), colour(7)], [colour(128), colour(1)]]
