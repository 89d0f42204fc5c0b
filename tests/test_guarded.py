"""Self-tests of tests/guarded.py on CPU tensors.  The "kernel" is plain torch indexing on the guarded buffer: each way of being
wrong that the guards exist for must fail, for the stated reason, and a correct writer must pass."""
import numpy as np
import pytest
import torch

from blind_image_denoising_amd import unet_laplacian as UL
from blind_image_denoising_amd import loss as LS
from blind_image_denoising_amd import _native as N
import guarded as G
from helpers import assert_close


def _served(session):
    """(buffer, guard bytes, body bytes) of the newest allocation"""
    r = session.records[-1]
    return r.big, r.guard, r.nbytes


def test_guard_rule():
    assert G.guard_bytes(0) == G.guard_bytes(1) == 64 << 10
    assert G.guard_bytes((64 << 10) + 1) == (64 << 10) + 4096
    assert G.guard_bytes(1 << 30) == 16 << 20 and G.guard_bytes(1 << 30, cap=1 << 20) == 1 << 20
    assert all(G.guard_bytes(n) % 4096 == 0 for n in (0, 1, 4095, 4097, 70001, 1 << 25))


def test_served_tensors_look_like_plain_ones():
    """shape, dtype, contiguity as torch.empty gives them.  The pointer: the guard is a multiple of 4096, so the tensor has, modulo
    4096, the address of the plain allocation that backs it (the host allocator itself promises 64 bytes, the device one 512)."""
    with G.guards(cpu=True) as s:
        for shape, dtype in (((2, 5, 7, 3), torch.float32), ((1, 1, 1, 1), torch.uint8), ((17,), torch.float16), ((3, 0, 2), torch.float64),
                             ((130, 1000), torch.int32), ((), torch.float32)):
            plain = torch.empty(shape, dtype=dtype)
            for make in (lambda: UL.torch.empty(shape, dtype=dtype), lambda: UL.torch.empty(*shape, dtype=dtype, device="cpu"),
                         lambda: UL.torch.empty_like(plain), lambda: UL.torch.zeros(shape, dtype=dtype),
                         lambda: UL.torch.zeros_like(plain), lambda: UL.torch.full(shape, 3, dtype=dtype)):
                t = make()
                big, guard, nbytes = _served(s)
                assert t.shape == plain.shape and t.dtype == plain.dtype and t.stride() == plain.stride() and t.is_contiguous()
                assert nbytes == plain.numel() * plain.element_size() and guard == G.guard_bytes(nbytes)
                if nbytes:
                    assert t.data_ptr() - big.data_ptr() == guard and t.data_ptr() % 4096 == big.data_ptr() % 4096
                    assert t.data_ptr() % 64 == plain.data_ptr() % 64 == 0
                assert big.numel() - (guard + nbytes) >= guard                      # the second guard starts at the last byte
        assert UL.torch.empty(3).dtype == torch.get_default_dtype() and UL.torch.full((2,), 2).dtype == torch.int64
        assert UL.torch.full((2,), 0.5).dtype == torch.float32 and UL.torch.full((2,), True).dtype == torch.bool
        assert (UL.torch.zeros((4, 4)) == 0).all() and (UL.torch.full((4, 4), 2.5) == 2.5).all() and (UL.torch.ones(5) == 1).all()
        assert (UL.torch.zeros_like(torch.ones(3)) == 0).all() and (UL.torch.full_like(torch.ones(3), 7.0) == 7).all()
    # without cpu=True host allocations are torch's own
    with G.guards() as s:
        UL.torch.empty((4,))
        assert not s.records


def test_everything_else_is_torch_itself():
    with G.guards(cpu=True):
        T = UL.torch
        assert T is not torch and T.Tensor is torch.Tensor and T.float32 is torch.float32 and T.cuda is torch.cuda and T.nn is torch.nn
        assert isinstance(T.empty(2), T.Tensor) and T.__version__ == torch.__version__ and T.from_numpy is torch.from_numpy
        assert T.empty((2,), pin_memory=False).shape == (2,)
        strided = torch.ones((4, 6)).t()
        assert T.empty_like(strided).stride() == torch.empty_like(strided).stride()      # not contiguous: torch's own
    assert UL.torch is torch


def test_unwritten_fill_is_nan_in_every_float_type_and_a_chosen_byte_in_integers():
    with G.guards(cpu=True) as s:
        for dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
            t = UL.torch.empty((3, 5), dtype=dtype)
            assert torch.isnan(t).all() and G.unwritten(t) == 15
            t[1] = 2.0
            assert G.unwritten(t) == 10
        for byte in G.INT_FILLS:
            s.int_byte = byte
            assert (UL.torch.empty((7,), dtype=torch.uint8) == byte).all()
            assert (UL.torch.empty((7,), dtype=torch.int32) == (0 if byte == 0 else -1)).all()
            assert (UL.torch.empty((7,), dtype=torch.bool) == bool(byte)).all()
        with pytest.raises(TypeError):
            G.unwritten(UL.torch.empty((7,), dtype=torch.uint8))


def test_a_correct_writer_passes():
    with G.guards(cpu=True) as s:
        x = G.dev(np.arange(15, dtype=np.float32).reshape(3, 5), device="cpu")
        u = G.dev(np.arange(7, dtype=np.uint8), device="cpu")
        out = UL.torch.empty_like(x)
        out.copy_(x * 2)
        o8 = UL.torch.empty((7,), dtype=torch.uint8)
        o8.copy_(u)
        assert len(s.records) == 4 and G.unwritten(out) == 0
        assert_close(out.numpy(), np.arange(15).reshape(3, 5) * 2.0)
    assert G.twice(lambda: G.dev(np.arange(7, dtype=np.uint8), device="cpu") + 1).tolist() == list(range(1, 8))


@pytest.mark.parametrize("dtype, shape", [(torch.float32, (3, 5)), (torch.uint8, (7,)), (torch.float16, (1, 3))])
def test_one_element_written_before_the_start_fails(dtype, shape):
    with pytest.raises(AssertionError, match=rf"guard band written: empty .* allocated at test_guarded:\d+, before the start, "
                                             rf"byte offset -{dtype.itemsize}$"):
        with G.guards(cpu=True) as s:
            t = UL.torch.empty(shape, dtype=dtype)
            t.fill_(1)
            big, guard, _ = _served(s)
            big[:guard].view(dtype)[-1] = 1


@pytest.mark.parametrize("dtype, shape", [(torch.float32, (3, 5)), (torch.uint8, (7,)), (torch.float16, (1, 3)), (torch.uint8, (1, 1, 1, 1))])
def test_one_element_written_after_the_end_fails(dtype, shape):
    """also where the tensor ends off a 4-byte boundary: the second guard starts at its last byte"""
    with pytest.raises(AssertionError, match=r"guard band written: empty .* allocated at test_guarded:\d+, after the end, byte offset 0$"):
        with G.guards(cpu=True) as s:
            t = UL.torch.empty(shape, dtype=dtype)
            t.fill_(1)
            big, guard, nbytes = _served(s)
            big[guard + nbytes:guard + nbytes + dtype.itemsize].view(dtype)[0] = 1


def test_a_store_far_behind_a_zeros_tensor_or_an_input_fails():
    with pytest.raises(AssertionError, match=r"zeros \(2, 3\) torch.float32 allocated at test_guarded:\d+, after the end, byte offset 60000$"):
        with G.guards(cpu=True) as s:
            UL.torch.zeros((2, 3))
            big, guard, nbytes = _served(s)
            big[guard + nbytes + 60000] = 0
    with pytest.raises(AssertionError, match=r"input \(5,\) torch.uint8 allocated at test_guarded:\d+, before the start, byte offset -1$"):
        with G.guards(cpu=True) as s:
            G.dev(np.zeros(5, np.uint8), device="cpu")
            big, guard, _ = _served(s)
            big[guard - 1] = 1


def test_one_float_element_left_unwritten_fails():
    with G.guards(cpu=True):
        out = UL.torch.empty((3, 5))
        out.view(-1)[:14] = 1.0
        assert G.unwritten(out) == 1
        with pytest.raises(AssertionError, match="non-finite"):
            assert_close(out.numpy(), np.ones((3, 5)))
        assert not np.array_equal(out.numpy(), np.ones((3, 5), np.float32))


def test_one_integer_element_left_unwritten_fails():
    def skips_the_last():
        out = UL.torch.empty((3, 5), dtype=torch.uint8)
        out.view(-1)[:14] = 1
        return out

    with pytest.raises(AssertionError, match=r"depends on the fill of unwritten integer memory .*1 bytes differ, the first at byte offset 14"):
        G.twice(skips_the_last, cpu=True)


def test_a_value_read_from_an_input_guard_fails():
    def halo_sum(a):
        """a 3-tap sum whose left tap at column 0 reads the element in front of the input instead of a zero"""
        with G.guards(cpu=True) as s:
            x = G.dev(a, device="cpu")
            big, guard, nbytes = _served(s)
            wide = big[guard - x.element_size():guard + nbytes].view(x.dtype)
            return (wide[:-1] + x + torch.cat([x[1:], torch.zeros(1, dtype=x.dtype)])).clone()

    a = np.arange(1, 7, dtype=np.float32)
    ref = np.convolve(a, np.ones(3), "same")
    with pytest.raises(AssertionError, match="non-finite"):
        assert_close(halo_sum(a).numpy(), ref)
    with pytest.raises(AssertionError, match=r"depends on the fill .*1 bytes differ, the first at byte offset 0"):
        G.twice(lambda: halo_sum(a.astype(np.uint8)))


def test_proxies_are_removed_on_exit_also_when_the_body_raises():
    import sys
    mods = [m for n, m in sys.modules.items() if n.startswith(G.PACKAGE) and getattr(m, "torch", None) is torch]
    assert len(mods) >= 30 and UL in mods
    scratch = N.scratch
    with G.guards(cpu=True):
        assert all(isinstance(m.torch, G._TorchProxy) for m in mods)
        assert "new_empty" in torch.Tensor.__dict__ and N.scratch is not scratch
        with G.guards(cpu=True) as inner:                                           # nested: the same context
            assert inner is G._SESSION[-1] and len(G._SESSION) == 1
    assert all(m.torch is torch for m in mods) and "new_empty" not in torch.Tensor.__dict__ and not G._SESSION and N.scratch is scratch
    with pytest.raises(ZeroDivisionError):
        with G.guards(cpu=True) as s:
            UL.torch.empty(3)
            big, guard, _ = _served(s)
            big[0] = 0                                                              # the body's own error is reported, not this
            1 / 0
    assert all(m.torch is torch for m in mods) and "new_zeros" not in torch.Tensor.__dict__ and not G._SESSION and N.scratch is scratch


def test_the_scratch_of_native_is_guarded():
    """_native.scratch imports torch inside the function; the tensor it sized comes back guarded, with the same shape and size.
    Needs no GPU, but the built library: the size comes from a host function of libbfcnn_hip.so."""
    plain, nbytes = N.scratch("bf_noise_level", "cpu", 1, 8, 8, 3)
    with G.guards(cpu=True) as s:
        t, n = N.scratch("bf_noise_level", "cpu", 1, 8, 8, 3)
        assert n == nbytes and t.shape == plain.shape and t.dtype == torch.float64 and G.unwritten(t) == t.numel()
        assert s.records[-1].what.startswith("scratch") and s.records[-1].nbytes == t.numel() * 8


def test_tensor_new_zeros_of_the_package_is_guarded():
    """loss.py sums its terms into terms[0].new_zeros(2)"""
    as_the_package = eval("lambda t: t.new_zeros(2)", LS.__dict__)                  # a caller whose globals are the module's
    with G.guards(cpu=True) as s:
        out = as_the_package(torch.ones(3))
        assert len(s.records) == 1 and s.records[0].what.startswith("new_zeros")
        mine = torch.ones(3).new_zeros(2)                                           # called from a test: torch's own
        assert len(s.records) == 1
    assert out.tolist() == [0, 0] and mine.tolist() == [0, 0]


def test_the_modules_named_in_also_are_served_and_restored():
    """the fixture names the test module: its own allocations are guarded too"""
    import types
    mine = types.ModuleType("a_test_module")
    mine.torch = torch
    with G.guards(cpu=True, also=(mine,)) as s:
        out = mine.torch.empty((3, 5))
        assert len(s.records) == 1 and G.unwritten(out) == 15 and isinstance(out, mine.torch.Tensor)
        out.fill_(0)
    assert mine.torch is torch
    with pytest.raises(AssertionError, match=r"allocated at test_guarded:\d+, after the end, byte offset 0$"):
        with G.guards(cpu=True, also=(mine,)) as s:
            mine.torch.full((3,), 7, dtype=torch.uint8)
            big, guard, nbytes = _served(s)
            big[guard + nbytes] = 7
    assert mine.torch is torch
