"""The dropout mask of the relu + pool epilogue (DESIGN.md 3.10 "dropout in the relu + pool epilogue"), restated in numpy: Philox4x32-10 on
the counter (lo32(e >> 2), hi32(e >> 2), 0, 0) under the key (lo32(seed), hi32(seed)); element e is kept iff output word e & 3 is >= thr.

CPU: the numpy Philox reproduces three known answers; the dropped share of 26 880 elements lies within 5 sigma of p; thr and scale
(F.dropout_params) for p in {0, 0.1, 0.5, 1 - 2^-24}; bad p and bad seeds are refused.
gpu: F.dropout_keep_mask (tgcn_dropout_keep_u8) is array_equal to the numpy mask -- an unaligned start, a counter carry into the high
word, an index beyond 2^40, seeds with a non-zero high half."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint64 arrays (values below 2^32) of one shape; key: two ints -> the four output words, uint64 arrays below 2^32"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def thr_of(p):
    return min(int(np.floor(p * 2.0 ** 32 + 0.5)), 2 ** 32 - 1)


def scale_of(p):
    return float(np.float32(1) / (np.float32(1) - np.float32(p)))


def keep_mask(seed, e, p):
    """bool array, True where the elements e (an array of non-negative integers below 2^63) are kept"""
    e = np.asarray(e, dtype=np.uint64)
    e4 = e >> np.uint64(2)
    zero = np.zeros_like(e4)
    words = np.stack(philox4x32_10((e4 & MASK32, e4 >> np.uint64(32), zero, zero), (seed & 0xFFFFFFFF, seed >> 32)), axis=-1)
    word = np.take_along_axis(words, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]
    return word >= np.uint64(thr_of(p))


def mask_values(seed, shape, p):
    """the multiplier m of every element of an output of `shape`, element index = flat index: scale where kept, 0 where dropped (float32)"""
    keep = keep_mask(seed, np.arange(int(np.prod(shape)), dtype=np.uint64), p).reshape(shape)
    return np.where(keep, np.float32(scale_of(p)), np.float32(0)).astype(np.float32)


KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_the_numpy_philox_reproduces_the_known_answers(ctr, key, want):
    got = philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
    assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("seed", [0, 1234, 2 ** 62 - 1])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_dropped_share_is_within_five_sigma_of_p(p, seed):
    count = 26880
    dropped = 1.0 - keep_mask(seed, np.arange(count), p).mean()
    sigma = np.sqrt(p * (1 - p) / count)
    print("p %.1f seed %d: dropped %.5f, %.2f sigma" % (p, seed, dropped, abs(dropped - p) / sigma))
    assert abs(dropped - p) <= 5 * sigma


def test_thr_and_scale():
    from tgcn_amd import functional as F
    want = {0: (0, 1.0), 0.1: (429496730, float(np.float32(1) / np.float32(0.9))), 0.5: (2 ** 31, 2.0), 1 - 2.0 ** -24: (2 ** 32 - 256, 2.0 ** 24)}
    for p, (thr, scale) in want.items():
        assert F.dropout_params(p) == (thr, scale) == (thr_of(p), scale_of(p)), p
    # float32(1) - float32(0.1) is not float32(0.9) in general: the rule is the float32 operations, in this order
    for p in (0.1, 0.2, 0.3, 0.7, 0.9, 1e-3, 0.999):
        assert F.dropout_params(p) == (thr_of(p), scale_of(p)), p
    assert thr_of(1 - 2.0 ** -40) == 2 ** 32 - 1          # the clamp -- which no accepted p reaches: such a p is 1 in float32, without a finite scale
    from tgcn_amd import _lib
    with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
        F.dropout_params(1 - 2.0 ** -40)


def test_bad_p_and_bad_seeds_are_refused():
    from tgcn_amd import _lib
    from tgcn_amd import functional as F
    for p in (-0.1, 1, 1.0, 1.5, float("nan"), None, "0.5", True):
        with pytest.raises(_lib.TgcnError, match=r"p is a real number in \[0, 1\)"):
            F.dropout_params(p)
    for seed in (-1, 2 ** 62, 1.5, "7", True):
        with pytest.raises(_lib.TgcnError, match="seed is None, an integer"):
            F.dropout_seed(seed, torch.device("cpu"))
    for seed in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(1)):
        with pytest.raises(_lib.TgcnError, match="one int64 element"):
            F.dropout_seed(seed, torch.device("cpu"))
    t = torch.tensor([5])
    assert F.dropout_seed(t, torch.device("cpu")).data_ptr() == t.data_ptr()
    assert F.dropout_seed(2 ** 62 - 1, torch.device("cpu")).tolist() == [2 ** 62 - 1]
    torch.manual_seed(3)
    a = F.dropout_seed(None, torch.device("cpu"))
    torch.manual_seed(3)
    assert torch.equal(a, F.dropout_seed(None, torch.device("cpu"))) and a.dtype == torch.int64 and 0 <= int(a) < 2 ** 62


SEEDS = [0, 1234, (0x1234567 << 32) | 0x89abcdef, 2 ** 62 - 1]
# the last: e >> 2 itself carries from 2^32 - 1 into the counter's high word inside the range
RANGES = [(0, 4099), (3, 101), (2 ** 32 - 37, 101), (2 ** 40 + 1, 64), (4 * 2 ** 32 - 37, 101)]


def test_the_ranges_hit_what_they_are_here_for():
    assert any(e0 % 4 for e0, _ in RANGES)                                                        # an unaligned start
    assert any(e0 < 2 ** 32 <= e0 + c - 1 for e0, c in RANGES)                                    # e crosses 32 bits
    assert any((e0 >> 2) < 2 ** 32 <= ((e0 + c - 1) >> 2) for e0, c in RANGES)                    # the counter's low word carries
    assert any((e0 >> 2) >> 32 for e0, c in RANGES)                                               # a counter with a high word
    assert any(s >> 32 for s in SEEDS)                                                            # a key with a high half


@gpu
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_the_device_mask_is_the_numpy_mask(p, seed, gpu_device):
    from tgcn_amd import functional as F
    for e0, count in RANGES:
        got = F.dropout_keep_mask(seed, e0, count, p, "cuda:0")
        assert got.dtype == torch.bool and tuple(got.shape) == (count,)
        want = keep_mask(seed, np.arange(e0, e0 + count, dtype=np.uint64), p)
        assert np.array_equal(got.cpu().numpy(), want), (e0, count)
    # the seed as a tensor on the device gives the same mask
    t = torch.tensor([seed], dtype=torch.int64, device="cuda:0")
    assert torch.equal(F.dropout_keep_mask(t, 3, 101, p, "cuda:0"), F.dropout_keep_mask(seed, 3, 101, p, "cuda:0"))
