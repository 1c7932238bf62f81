"""Guarded device buffers for tests that call a C entry point directly: every output (and workspace) is a slice of a larger
allocation with GUARD sentinel elements before and after it, prefilled with NaN; after the call the sentinels must be unchanged bit
for bit -- a write past either end is seen without any fault -- and no output element may still be NaN (an element the kernel never
wrote).  The first element of every slice is 16-byte aligned (torch's allocations are, and GUARD elements are a multiple of 16 B)."""
import torch

from tests.util import OP_RTOL, assert_close, record

GUARD = 64
NAN16 = 0x7FC0       # bf16 NaN (split planes)
_INT = {torch.float32: torch.int32, torch.int16: torch.int16}


def _sentinel(dtype, device):
    bits = torch.arange(GUARD, dtype=torch.int64) * 2654435761 % 32749 + 1
    if dtype == torch.float32:      # finite fp32 patterns, all different
        return (bits.to(torch.int32) + 0x4B000000).to(device)
    return bits.to(torch.int16).to(device)


class Guards:
    def __init__(self, device="cuda"):
        self.device = device
        self.items = []     # (name, whole buffer as ints, payload view, may hold NaN)

    def _new(self, name, numel, dtype, nan_ok):
        assert (GUARD * torch.empty(0, dtype=dtype).element_size()) % 16 == 0
        buf = torch.empty(numel + 2 * GUARD, dtype=dtype, device=self.device)
        ib = buf.view(_INT[dtype])
        s = _sentinel(dtype, self.device)
        ib[:GUARD] = s
        ib[GUARD + numel:] = s
        t = buf[GUARD:GUARD + numel]
        assert t.data_ptr() % 16 == 0
        self.items.append((name, ib, t, nan_ok))
        return t

    def out(self, name, *shape):
        """NaN-filled fp32 output of the given shape"""
        n = 1
        for s in shape:
            n *= s
        t = self._new(name, n, torch.float32, False)
        t.fill_(float("nan"))
        return t.view(*shape)

    def planes(self, name, n):
        """NaN-filled split planes (2, n) of int16"""
        t = self._new(name, 2 * n, torch.int16, True)
        t.fill_(NAN16)
        return t.view(2, n)

    def ws(self, name, nbytes):
        """workspace of exactly nbytes (a multiple of 4), NaN-filled; scratch may keep NaN"""
        assert nbytes % 4 == 0
        t = self._new(name, nbytes // 4, torch.float32, True)
        t.fill_(float("nan"))
        return t, nbytes

    def state(self, name, value):
        """in-place state (optimiser arenas): the given CPU tensor, guarded"""
        t = self._new(name, value.numel(), torch.float32, False)
        t.copy_(value.reshape(-1))
        return t.view(value.shape)

    def check(self):
        torch.cuda.synchronize()
        for name, ib, t, nan_ok in self.items:
            s = _sentinel(ib.dtype if ib.dtype == torch.int16 else torch.float32, self.device)
            n = t.numel()
            assert torch.equal(ib[:GUARD], s), f"{name}: the {GUARD} elements before the buffer were written"
            assert torch.equal(ib[GUARD + n:], s), f"{name}: the {GUARD} elements after the buffer were written"
            if not nan_ok:
                bad = torch.isnan(t)
                assert not bad.any(), f"{name}: {int(bad.sum())} of {n} elements never written (first at {int(bad.nonzero()[0])})"


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    """fp32 tensors equal bit for bit (distinguishes -0.0 from 0.0, compares NaN payloads)"""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ---- what the tests of the small kernels share -----------------------------------------------------------------------------------
def api():
    """(_lib module, ops module, loaded library)"""
    from vae_play_amd import _lib, ops
    return _lib, ops, _lib.load()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tensor_close(got, ref, what):
    """a tensor against its fp64 reference: OP_RTOL in rel_err's norm, the measured error printed and recorded"""
    e = assert_close(got.reshape(ref.shape), ref, OP_RTOL, what)
    print(f"{what}: {e:.3e}")
    return e


def scalar_close(got, ref, what, denom=None, tol=OP_RTOL):
    """|got - ref| <= tol * |ref| (or tol * denom), element by element for a tensor of sums"""
    got, ref = torch.as_tensor(got).detach().double().cpu().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = ref.abs() if denom is None else torch.as_tensor(denom).double().reshape(-1)
    e = ((got - ref).abs() / (d + 1e-30)).max().item()
    record(what, e)
    print(f"{what}: {e:.3e}")
    assert e <= tol, f"{what}: {got.tolist()[:4]} vs {ref.tolist()[:4]}: rel err {e:.3e} > {tol:.1e}"
    return e
