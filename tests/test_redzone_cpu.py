"""CPU: the guard-band instrument (tests/redzone.py) can fail.  Each of its detectors — a write outside the payload, an
element left unwritten, a modified input — is shown to fire on CPU tensors, and patched_allocations to restore torch's
factories on every exit path.  No GPU is involved and nothing is provoked."""
import pytest

torch = pytest.importorskip('torch')

import redzone


def test_layout():
    for shape, dtype in (((3, 5), torch.float64), ((100000,), torch.float32), ((7,), torch.int64), ((2, 3), torch.complex128)):
        g = redzone.guarded(shape, dtype, 'cpu')
        assert g.t.shape == shape and g.t.dtype == dtype and g.t.is_contiguous()
        assert g.guard % 256 == 0 and g.guard >= 64 * 1024 and g.guard >= g.nbytes
        assert g.base.numel() == 2 * g.guard + g.nbytes and g.base.dtype == torch.uint8
        assert g.t.data_ptr() == g.base.data_ptr() + g.guard
        assert bool((g.base[:g.guard] == 0xA5).all()) and bool((g.base[g.guard + g.nbytes:] == 0xA5).all())
        assert bool((g.payload == 0xFF).all())
        g.check()
        assert g.unwritten() == g.nbytes // (8 if dtype != torch.float32 else 4)
    g = redzone.guarded((4,), torch.float64, 'cpu')
    assert bool(torch.isnan(g.t).all())                       # all-ones bytes: a NaN for floats ...
    assert redzone.guarded((4,), torch.int64, 'cpu').t.tolist() == [-1] * 4       # ... and -1 for counts
    assert redzone.guarded((4,), torch.float32, 'cpu', fill=0).t.tolist() == [0.0] * 4


@pytest.mark.parametrize('where', ['before', 'after'])
def test_a_write_one_byte_outside_the_payload_is_reported(where):
    g = redzone.guarded((33,), torch.float32, 'cpu')
    g.t.fill_(1.0)
    g.check(written=True)
    off = g.guard - 1 if where == 'before' else g.guard + g.nbytes
    g.base[off] = 0                                            # through the base buffer: one byte next to the payload
    with pytest.raises(AssertionError) as err:
        g.check()
    msg = str(err.value)
    assert ('front guard' in msg and '-1' in msg) if where == 'before' else ('back guard' in msg and '+0' in msg), msg
    assert '1 byte(s) touched' in msg


def test_a_2x_overrun_is_reported_with_its_extent():
    """the overrun this project has had: a float64 result into a float32 buffer lands wholly inside the back guard"""
    g = redzone.guarded((1000,), torch.float32, 'cpu')
    g.base[g.guard:g.guard + 2 * g.nbytes] = 0
    with pytest.raises(AssertionError, match=r'back guard: 4000 byte\(s\) touched, first at payload end\+0, last at \+3999'):
        g.check()


def test_an_unwritten_element_is_reported():
    for dtype, value in ((torch.float64, 2.5), (torch.float32, 2.5), (torch.int64, 3), (torch.complex128, 1 + 2j)):
        g = redzone.guarded((5, 7), dtype, 'cpu')
        g.t.fill_(value)
        g.check(written=True)
        g.refill(0xFF)
        g.t.fill_(value)
        g.payload[-g.t.element_size():] = 0xFF                 # the last element never written
        g.check()                                              # the guards are intact
        with pytest.raises(AssertionError, match='still hold the prefill 0xFF'):
            g.check(written=True)
    g = redzone.guarded((8,), torch.float64, 'cpu', fill=0x00)
    g.t[:7] = 1.0
    with pytest.raises(AssertionError, match='1 element.*0x00'):
        g.check(written=True)


def test_a_modified_input_is_reported():
    x = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    x[0, 0, 0] = float('nan')                                  # NaN != NaN must not read as a change
    f = redzone.frozen(x)
    f.check()
    x[1, 2, 3] = -x[1, 2, 3]
    with pytest.raises(AssertionError, match='was modified: 1 word'):
        f.check()
    z = torch.zeros(4, dtype=torch.float32)
    f = redzone.frozen(z)
    z[2] = -0.0                                                # equal as a float, different bits
    with pytest.raises(AssertionError, match='was modified'):
        f.check()


def test_patched_allocations_restores_the_factories():
    orig = [getattr(torch, n) for n in ('empty', 'zeros', 'empty_like', 'zeros_like')]
    with pytest.raises(RuntimeError, match='boom'):
        with redzone.patched_allocations():
            assert torch.empty is not orig[0]
            a = torch.empty(3)                                 # a CPU result passes through untouched
            assert a.shape == (3,) and torch.zeros_like(a).tolist() == [0.0] * 3
            raise RuntimeError('boom')
    assert [getattr(torch, n) for n in ('empty', 'zeros', 'empty_like', 'zeros_like')] == orig
    with redzone.patched_allocations() as reg:
        torch.zeros((2, 2))
        assert reg == []                                       # CUDA results only
    assert torch.empty is orig[0]
