"""CPU: the oracle's Philox4x32-10 (oracle/samplers_ref.py) against the published known-answer vectors of Random123
(Salmon et al. 2011, kat_vectors: philox4x32 10).  The device stream is pinned against this oracle only, so the oracle
itself must be pinned against something it does not share an author with."""
import numpy as np
import pytest

from oracle import samplers_ref

KAT = [
    ((0, 0, 0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 6, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('inp,out', KAT)
def test_philox4x32_10_known_answers(inp, out):
    got = samplers_ref.philox4x32_10(*inp)
    assert tuple(int(np.asarray(g).reshape(-1)[0]) for g in got) == out
    # vectorised over the first counter word: the same answer in every lane that holds the vector's c0
    c0 = np.array([inp[0], inp[0] ^ 1, inp[0]], dtype=np.uint32)
    lanes = samplers_ref.philox4x32_10(c0, *inp[1:])
    assert tuple(int(g[0]) for g in lanes) == out and tuple(int(g[2]) for g in lanes) == out
    assert tuple(int(g[1]) for g in lanes) != out


def test_philox_normal_follows_the_counter_layout():
    """counter (quad, step lo, member mod 2^32, step hi), key (seed lo, seed hi)"""
    seed, member, step, n = 0xF234567890ABCDEF, 12, 2 ** 32 + 3, 16
    _, raw = samplers_ref.philox_normal(seed, member, step, n)
    for quad in range(n // 4):
        want = samplers_ref.philox4x32_10(quad, 3, member, 1, 0x90ABCDEF, 0xF2345678)
        assert [int(np.asarray(w).reshape(-1)[0]) for w in want] == [int(r) for r in raw[4 * quad:4 * quad + 4]]


def test_philox_normal_member_id_is_taken_modulo_2_32():
    """the device's counter word is 32 bits wide (include/qgx.h): ids that differ by 2^32 draw the same stream, where
    this function used to raise OverflowError"""
    for member in (0, 1, 2 ** 32 - 1):
        a, ra = samplers_ref.philox_normal(5, member, 7, 64)
        b, rb = samplers_ref.philox_normal(5, member + 2 ** 32, 7, 64)
        assert np.array_equal(ra, rb) and np.array_equal(a, b)
    assert not np.array_equal(samplers_ref.philox_normal(5, 2 ** 32 - 1, 7, 64)[1], samplers_ref.philox_normal(5, 0, 7, 64)[1])
