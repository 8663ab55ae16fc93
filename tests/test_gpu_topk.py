"""rnnl_topk_rows on the GPU against its numpy restatement (tests/topk_ref.py):
index, score bits and valid must be equal exactly.

The kernel has one code path for every row length and k; what differs by data
is the end of the selection (fewer than k eligible / every key equal to the
k-th belongs to the result / only the first ones by entity id do), and each row
content below is run at every shape that can hold it: one entity, k above |E|,
the wave (64), workgroup (256) and 4 x 256-entity loop-step (1024) boundaries
and their neighbours, the sort buffer's capacity (k = 1024), the FB15k-237
row length, and the graph-size ceiling of 524,288 entities.
"""
import numpy as np
import pytest
import torch

import topk_ref

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 1), (3, 5, 10),
          (4, 63, 7), (4, 64, 7), (4, 65, 7),
          (4, 255, 64), (4, 256, 64), (4, 257, 64),
          (4, 1024, 1024), (4, 1025, 1024),
          (8, 4099, 100),
          (64, 14541, 1), (64, 14541, 10), (64, 14541, 1024),
          (2, 524288, 1024)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _tied_scores(rng, n, E):
    """Random scores on a coarse grid: many exact ties."""
    return (rng.integers(-64, 64, size=(n, E)) / 8.0).astype(np.float32)


def _true_topk(score, k):
    return topk_ref.topk_ref(score, None, None, None, k)[0]


# ---- row contents: (rng, n, E, k) -> (score, mask, flag, keep), or None when the shape cannot hold it
def all_equal(rng, n, E, k):
    vals = np.array([0.5, -2.0, 0.0, -0.0, np.inf, -np.inf, 1e-40, 3.0], dtype=np.float32)
    return np.repeat(vals[np.arange(n) % len(vals)][:, None], E, 1), None, None, None


def three_values(rng, n, E, k):
    if E < 3:
        return None
    score = rng.choice(np.array([-1.5, 0.25, 7.0], dtype=np.float32), size=(n, E))
    score[:, :3] = [-1.5, 0.25, 7.0]  # every value occurs
    if E > k >= 3:
        # row 0: fewer than k above the middle value, so the k-th place falls inside its tie run
        score[0] = np.where(np.arange(E) % (E // (k - 1) + 1) == 1, 7.0, 0.25)
        score[0, 0] = -1.5
    return score, None, None, None


def low_bits(rng, n, E, k):
    bits = (0x3F800000 + rng.integers(0, 4, size=(n, E))).astype(np.uint32)
    bits[1::2] |= 0x80000000  # negative rows: the key order of the low bits flips
    return bits.view(np.float32), None, None, None


def specials(rng, n, E, k):
    score = (rng.standard_normal((n, E)) * 10.0 ** rng.integers(-3, 4, size=(n, E))).astype(np.float32)
    pool = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x000FFFFF,
                     0x807FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    pick = rng.random((n, E)) < 0.4
    score[pick] = pool[rng.integers(0, len(pool), size=int(pick.sum()))]
    return score, None, None, None


def ascending(rng, n, E, k):
    return (np.arange(E, dtype=np.float32)[None, :] - np.arange(n, dtype=np.float32)[:, None] * 3), None, None, None


def descending(rng, n, E, k):
    return ascending(rng, n, E, k)[0][:, ::-1].copy(), None, None, None


def mask_counts(rng, n, E, k):
    """mask leaving 0, k - 1, k and k + 1 eligible (as far as |E| allows)."""
    score = _tied_scores(rng, n, E)
    mask = np.zeros((n, E), dtype=bool)
    for i in range(n):
        c = min(E, [0, k - 1, k, k + 1][i % 4])
        mask[i, rng.permutation(E)[:c]] = True
    return score, mask, None, None


def flag_top(rng, n, E, k):
    """flag removing the whole true top-k."""
    score = _tied_scores(rng, n, E)
    flag = np.ones((n, E), dtype=bool)
    top = _true_topk(score, k)
    for i in range(n):
        flag[i, top[i][top[i] >= 0]] = False
    return score, None, flag, None


def keep_cases(rng, n, E, k):
    """keep re-admitting one flagged entity / one flagged-and-masked entity
    (which stays out) / nothing (out of range)."""
    score, _, flag, _ = flag_top(rng, n, E, k)
    mask = rng.random((n, E)) < 0.8
    top = _true_topk(score, k)
    keep = np.zeros(n, dtype=np.int64)
    for i in range(n):
        first = int(top[i, 0])
        if i % 3 == 0:
            keep[i], mask[i, first] = first, True
        elif i % 3 == 1:
            keep[i], mask[i, first] = first, False
        else:
            keep[i] = [E, -1, 1 << 40, -(1 << 40)][(i // 3) % 4]
    return score, mask, flag, keep


CONTENTS = [all_equal, three_values, low_bits, specials, ascending, descending, mask_counts, flag_top, keep_cases]


def _run(dev, score, mask, flag, keep, k):
    from rnnlogic_amd.predictors import topk_rows
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    out = topk_rows(t(score), t(mask), t(flag), t(keep), k)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("content", CONTENTS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dk%d" % s)
def test_topk_equals_reference(shape, content, dev):
    n, E, k = shape
    rng = np.random.default_rng(1000 * E + k)
    case = content(rng, n, E, k)
    if case is None:
        return  # (3, 1, 1) holds no three distinct values
    score, mask, flag, keep = case
    want = topk_ref.topk_ref(score, mask, flag, keep, k)
    got = _run(dev, score, mask, flag, keep, k)
    topk_ref.assert_equal(got, want, "%s %s" % (content.__name__, shape))
    index, value, valid = got
    if content is all_equal:
        assert (index == np.where(np.arange(k) < min(k, E), np.arange(k), -1)[None, :]).all()
    if content is specials:
        assert not np.isnan(value).any()
    if content is keep_cases:
        for i in range(n):
            # the kept entity is back at the top; masked or out of range, it stays out
            assert (index[i, 0] == keep[i]) == (i % 3 == 0)
            assert i % 3 == 0 or keep[i] not in index[i]


def test_null_arguments_repeat_and_stream(dev):
    """Each of mask, flag and keep as NULL; keep without flag is ignored; two
    calls give the same bits; a non-default stream."""
    from rnnlogic_amd.predictors import topk_rows
    n, E, k = 6, 777, 33
    rng = np.random.default_rng(5)
    score, mask, flag, keep = keep_cases(rng, n, E, k)
    first = None
    for m, f, kp in [(None, None, None), (mask, None, None), (None, flag, None), (None, flag, keep),
                     (mask, flag, None), (mask, None, keep), (mask, flag, keep)]:
        want = topk_ref.topk_ref(score, m, f, kp if f is not None else None, k)
        got = _run(dev, score, m, f, kp, k)
        topk_ref.assert_equal(got, want, "nulls")
        first = got
    again = _run(dev, score, mask, flag, keep, k)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    side = torch.cuda.Stream(dev)
    ts, tm, tf, tk = [torch.from_numpy(x).to(dev) for x in (score, mask, flag, keep)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = topk_rows(ts, tm, tf, tk, k)
    side.synchronize()
    for a, b in zip(first, out):
        assert a.tobytes() == b.cpu().numpy().tobytes()


def test_wrapper_rejects_bad_k(dev):
    from rnnlogic_amd.predictors import topk_rows
    score = torch.zeros((2, 5), device=dev)
    for k in (0, 1025):
        with pytest.raises(ValueError):
            topk_rows(score, None, None, None, k)
    index, value, valid = topk_rows(score[:0], None, None, None, 3)  # no rows: no launch
    assert index.shape == (0, 3) and value.shape == (0, 3) and valid.shape == (0,)
