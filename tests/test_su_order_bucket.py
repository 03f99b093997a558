"""The heading order of an integer-form launch (csrc/tdr_score_su.hip: tdr_su_order, through tdr_k_su_order) as a one-pass
stable bucket sort — tdr_config_tuning("su_order_bucket") = 1 — against rocPRIM's stable sort (= 0) and a NumPy model: the slot
list, the keys and the counts are the same BYTES.  A stable sort by key has one answer.  Run with `pytest -m gpu`.

The model.  Position t of the caller's order holds particle p = perm[t].  Its key is its heading bin — headings sit at exact bin
values 2 pi b / nb — unless the particles at positions t - 32 and t + 32 (clamped) lie more than `span` cells apart in x or y
(or one of them is NaN): then it is nb, "sparse".  Bin b's particles take slots [slot_start[b], + cnt[b]) in ascending position,
-1 follows up to the next multiple of 64, the sparse particles follow the bins, unpadded, in position order, and counts =
{padded slots of the bins, sparse particles, both}.  Every call gets a workspace the test has filled with 0x7F bytes: the bucket
sort writes nothing behind counts[2], the rocPRIM path fills the whole list with -1 first; tdr_k_su_order says which ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEG = 512                                    # positions per segment of the bucket sort (SU_SEG)
NS = (1, 63, 64, 65, 511, 512, 513, 4097, 20_000, 70_001)
NBS = (1, 4, 100, 256, 4095)
DISTS = ("one bin", "round robin", "all sparse", "all dense", "90/10 mix", "a NaN position", "a key across a segment border")
UNTOUCHED = 0x7F7F7F7F


@pytest.fixture(scope="module")
def k():
    import torch
    from top_down_renderer_amd.kernels import HipKernels

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    kk = HipKernels()
    before = kk.tuning("su_order_bucket")
    assert before == 1                       # the default
    yield kk
    kk.tuning("su_order_bucket", before)


def bucket_rule(n, nb):
    """The rule of shapes (tdr_score_su.hip): the table of one word per (segment, key) stays within 4 n + 65536 words."""
    return -(-n // SEG) * (nb + 1) <= 4 * n + 65536


def make_case(n, nb, dist, rng):
    """Per POSITION of the caller's order: heading bin, x, y; and the span."""
    t = np.arange(n)
    x = np.full(n, 50.0, np.float32)
    y = np.full(n, 50.0, np.float32)
    span = 0.0
    if dist == "one bin":
        bins = np.full(n, nb // 2)
    elif dist == "round robin":              # every segment holds every key (where it is long enough)
        bins = t % nb
    elif dist == "all sparse":
        bins = rng.integers(0, nb, n)
        x = (t * 1.0).astype(np.float32)
        y = (t * 2.0).astype(np.float32)
        span = 1e-3
    elif dist == "all dense":
        bins = rng.integers(0, nb, n)
        x = rng.uniform(0.0, 1000.0, n).astype(np.float32)
    elif dist == "90/10 mix":
        bins = rng.integers(0, nb, n)
        x = rng.uniform(49.0, 51.0, n).astype(np.float32)
        y = rng.uniform(49.0, 51.0, n).astype(np.float32)
        far = rng.random(n) < 0.1 / 2        # every far particle makes two positions sparse
        x[far] = (1000.0 + 10.0 * t[far]).astype(np.float32)
        span = 8.0
    elif dist == "a NaN position":
        bins = rng.integers(0, nb, n)
        x[0] = np.nan                        # the lower neighbour of positions 0..32
        if n > 100:
            y[100] = np.nan
        span = 8.0
    else:                                    # a run of one key over the border between segments 0 and 1 (n > 512)
        bins = (t * 7 + 3) % nb
        bins[SEG - 20:SEG + 20] = nb - 1
    return bins.astype(np.int64), x, y, span


def model(bins, x, y, span, perm, nb):
    n = len(bins)
    t = np.arange(n)
    keys = bins.copy()
    if span > 0:
        ta, tb = np.maximum(t - 32, 0), np.minimum(t + 32, n - 1)
        with np.errstate(invalid="ignore"):
            near = (np.abs(x[tb] - x[ta]) <= np.float32(span)) & (np.abs(y[tb] - y[ta]) <= np.float32(span))
        keys[~near] = nb
    cnt = np.bincount(keys, minlength=nb + 1)
    padded = cnt.copy()
    padded[:nb] = (cnt[:nb] + 63) // 64 * 64
    slot_start = np.cumsum(padded) - padded
    total = int(padded.sum())
    slots = np.full(total, -1, np.int32)
    order = np.argsort(keys, kind="stable")
    start = np.cumsum(cnt) - cnt
    sk = keys[order]
    slots[slot_start[sk] + (np.arange(n) - start[sk])] = perm[order]
    counts = np.array([total - cnt[nb], cnt[nb], total], np.int32)
    return slots, keys.astype(np.int32), counts


def states(k, bins, x, y, perm, nb):
    """[7][n] floats: init_x_px, init_y_px, dx_m, dy_m, theta, scale, have_init — particle perm[t] sits at position t."""
    n = len(bins)
    st = np.zeros((7, n), np.float32)
    st[0, perm] = x
    st[1, perm] = y
    st[4, perm] = (2.0 * np.pi * bins / nb).astype(np.float32)
    st[5] = 1.0
    st[6] = 1.0
    return k.to_device(st)


def run(k, st, n, nb, span, perm_dev, mode, workspace=None):
    import torch
    assert k.tuning("su_order_bucket", mode) == mode
    need = int(k.lib.tdr_k_su_order_workspace_ints(n, nb))
    if workspace is None:
        workspace = k.empty((need,), torch.int32)
    workspace[:need] = UNTOUCHED
    slots, keys, counts, bucket = k.su_order(st, n, nb, span, perm=perm_dev, workspace=workspace)
    k.synchronize()
    assert bucket == (mode == 1 and bucket_rule(n, nb)), (n, nb, mode, "the path the rule of shapes names")
    return slots.cpu().numpy(), keys.cpu().numpy(), counts.cpu().numpy()


def check_case(k, n, nb, dist, with_perm, rng, workspace=None):
    bins, x, y, span = make_case(n, nb, dist, rng)
    perm = rng.permutation(n).astype(np.int32) if with_perm else np.arange(n, dtype=np.int32)
    want_slots, want_keys, want_counts = model(bins, x, y, span, perm, nb)
    if dist == "all sparse" and n > 1:
        assert want_counts[0] == 0 and want_counts[1] == n
    if dist in ("all dense", "one bin", "round robin"):
        assert want_counts[1] == 0
    if dist == "a NaN position" and n > 1:
        assert want_keys[0] == nb                      # the particle at the NaN's side comes out sparse
    st = states(k, bins, x, y, perm, nb)
    perm_dev = k.to_device(perm) if with_perm else None
    got = {mode: run(k, st, n, nb, span, perm_dev, mode, workspace) for mode in (1, 0)}
    tag = (n, nb, dist, with_perm)
    used = int(want_counts[2])
    for mode in (1, 0):
        slots, keys, counts = got[mode]
        assert np.array_equal(counts, want_counts), (tag, mode, counts, want_counts)
        assert np.array_equal(keys, want_keys), (tag, mode)
        assert np.array_equal(slots[:used], want_slots), (tag, mode)
    # the two paths, byte for byte (the words in use; behind them the bucket sort writes nothing, rocPRIM's path its fill)
    assert got[1][0][:used].tobytes() == got[0][0][:used].tobytes(), tag
    assert got[1][1].tobytes() == got[0][1].tobytes() and got[1][2].tobytes() == got[0][2].tobytes(), tag
    assert (got[0][0][used:] == -1).all(), tag
    behind = got[1][0][used:]
    assert (behind == (UNTOUCHED if bucket_rule(n, nb) else -1)).all(), (tag, "the path the rule of shapes names")


@pytest.mark.parametrize("nb", NBS)
def test_bucket_order_is_the_stable_sort(k, nb):
    rng = np.random.default_rng(9000 + nb)
    for n in NS:
        for dist in DISTS:
            for with_perm in (False, True):
                check_case(k, n, nb, dist, with_perm, rng)


def test_shapes_above_the_table_bound_take_the_rocprim_path(k):
    """4095 headings: a small filter's table is in proportion, a large one's is not — and both orders are the model's."""
    assert bucket_rule(4097, 4095) and not bucket_rule(20_000, 4095) and not bucket_rule(70_001, 4095)
    assert bucket_rule(70_001, 256) and bucket_rule(1_000_000, 1023) and not bucket_rule(1_000_000, 4095)
    rng = np.random.default_rng(77)
    for n in (4097, 20_000):
        check_case(k, n, 4095, "90/10 mix", True, rng)   # (run() asserts which path ran)
    # the workspace never shrinks as n grows, across the bound too: one sized for n holds every launch of fewer particles
    sizes = [int(k.lib.tdr_k_su_order_workspace_ints(n, 4095)) for n in (1, 4097, 16_383, 16_385, 20_000, 70_001)]
    assert sizes == sorted(sizes), sizes


def test_the_workspace_is_the_size_function_s_answer(k):
    """A workspace of exactly tdr_k_su_order_workspace_ints words with canary words behind it, for a bucket-sorted shape, a
    Cartesian (two-key) one and one the rule leaves to rocPRIM; the scoring workspaces cover the same carve."""
    import torch
    CANARY, WORDS = 0x5CA1AB1E, 4096
    rng = np.random.default_rng(5)
    for n, nb in ((20_000, 256), (4097, 1), (513, 4095), (20_000, 4095)):
        need = int(k.lib.tdr_k_su_order_workspace_ints(n, nb))
        assert need > 0
        buf = torch.full((need + WORDS,), CANARY, dtype=torch.int32, device=k.device)
        check_case(k, n, nb, "90/10 mix", True, rng, workspace=buf)
        assert (buf[need:] == CANARY).all().item(), (n, nb)
    # the polar and the Cartesian scoring workspaces hold the order's carve, the table included
    assert int(k.lib.tdr_score_workspace_floats(3, 256, 256, 100_000, 100_000)) >= int(k.lib.tdr_k_su_order_workspace_ints(100_000, 256))
    assert int(k.lib.tdr_score_cart_workspace_floats(3, 64, 64, 100_000, 100_000)) >= int(k.lib.tdr_k_su_order_workspace_ints(100_000, 1))
