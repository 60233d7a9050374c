"""Guard bands around exact-size scratch and output buffers ("The scratch contract"), as a plain
module (not a conftest).  The product's nn._ops.Workspaces hands a kernel `torch.empty(max(nbytes, 256))` and only grows, so
in a test process a buffer usually has slack behind it; here every buffer is a view of EXACTLY the bytes asked for, 256-byte
aligned inside one backing allocation [guard | interior | guard] whose guards (and fresh interior) hold the int32 pattern
0x7FC0BEEF, the quiet NaN of tests/test_hip_mask_edges.py and tests/_tilegrid_cases.py.  A write past either end lands in
the test's own memory and `check()` names it; a read of scratch the call did not write yields that NaN.  Nothing here
provokes anything: the guards are passive.  tests/test_scratch_guard_cpu.py shows on CPU tensors that the checks bite."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from nn import _hip, _ops  # noqa: E402

PATTERN = 0x7FC0BEEF
ALIGN = 256
MIN_GUARD = 1 << 20                      # bytes on each side, and at least a quarter of the interior


def _pattern_bytes(n: int, device) -> torch.Tensor:
    """the n bytes a pattern-filled region that starts on a word boundary holds"""
    return torch.full(((n + 3) // 4,), PATTERN, dtype=torch.int32, device=device).view(torch.uint8)[:n]


def _last_true(d: torch.Tensor) -> int:
    """index of the last True of a 1-d bool tensor, -1 when there is none"""
    if d.numel() == 0 or not bool(d.any()):
        return -1
    return d.numel() - 1 - int(d.flip(0).to(torch.uint8).argmax())


class Block:
    """one backing allocation [guard | interior of exactly nbytes | guard]; `view` is the interior as uint8"""

    def __init__(self, name: str, nbytes: int, device, zero: bool = False):
        self.name, self.nbytes, self.zero = name, int(nbytes), zero
        self.guard = -(-max(MIN_GUARD, (self.nbytes + 3) // 4) // ALIGN) * ALIGN
        total = 2 * self.guard + -(-self.nbytes // 4) * 4 + ALIGN
        self.backing = torch.full((total // 4,), PATTERN, dtype=torch.int32, device=device).view(torch.uint8)
        self.off = self.guard + (-(self.backing.data_ptr() + self.guard)) % ALIGN      # a multiple of 4: words stay words
        self.view = self.backing[self.off:self.off + self.nbytes]
        if zero:
            self.view.zero_()

    def refill(self) -> None:
        self.view.copy_(_pattern_bytes(self.nbytes, self.view.device))

    def check(self) -> None:
        """AssertionError naming the buffer, the offset (relative to the interior's first byte) and the number of guard
        bytes that no longer hold the pattern"""
        end = self.off + self.nbytes
        head = self.backing[:self.off] != _pattern_bytes(self.off, self.backing.device)
        skip = end % 4                                               # the interior may end inside a word
        tail_all = _pattern_bytes(self.backing.numel() - end + skip, self.backing.device)[skip:]
        tail = self.backing[end:] != tail_all
        nh, nt = int(head.sum()), int(tail.sum())
        if nh or nt:
            first = int(head.to(torch.uint8).argmax()) - self.off if nh else self.nbytes + int(tail.to(torch.uint8).argmax())
            raise AssertionError(f"{self.name} ({self.nbytes} bytes): {nh + nt} guard bytes written ({nh} before, {nt} behind "
                                 f"the buffer), the first at offset {first} from the buffer's start")

    def high_water(self) -> int:
        """offset of the last interior byte that differs from the fresh fill (pattern, or zero for a zeroed buffer); -1 when
        the interior is untouched"""
        if self.zero:
            return _last_true(self.view != 0)
        return _last_true(self.view != _pattern_bytes(self.nbytes, self.view.device))


def _capturing(device) -> bool:
    return torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()


class GuardedWorkspaces(_ops.Workspaces):
    """nn._ops.Workspaces whose buffers are exact: `get` keeps one CURRENT buffer per (tag, device), as the product does, but
    it is a view of exactly `nbytes`; a request of another size checks the current buffer's guards and makes (or takes up
    again) the exact one of that size.  Buffers of earlier sizes stay alive and are checked by check() too, so a captured
    graph that points into them stays valid and a request that repeats a size gets the same storage back."""

    def __init__(self):
        super().__init__()
        self.blocks = {}                 # (tag, device, nbytes) -> Block of a `get`
        self.fixed_blocks = {}           # (tag, device, key) -> Block of a `zeroed`

    def get(self, tag: str, nbytes: int, device) -> torch.Tensor:
        nbytes = int(nbytes)
        key = (tag, str(device))
        cur = self.bufs.get(key)
        if cur is not None and cur.numel() == nbytes:
            return cur
        if cur is not None:
            largest = max(k[2] for k in self.blocks if k[:2] == key)
            if self.frozen and nbytes > largest:
                raise _hip.StrotssHipError(f"workspace {tag!r} is frozen under a captured graph at {largest} bytes and "
                                           f"cannot grow to {nbytes}")
            if not _capturing(device):
                self.blocks[key + (cur.numel(),)].check()
        blk = self.blocks.get(key + (nbytes,))
        if blk is None:
            assert not _capturing(device), f"workspace {tag!r}: {nbytes} bytes first asked for under capture (no eager step did)"
            blk = self.blocks[key + (nbytes,)] = Block(f"workspace {tag!r}", nbytes, device)
        self.bufs[key] = blk.view
        return blk.view

    def zeroed(self, tag: str, key, nbytes: int, device) -> torch.Tensor:
        key = (tag, str(device), key)
        blk = self.fixed_blocks.get(key)
        if blk is None:
            blk = self.fixed_blocks[key] = Block(f"zeroed workspace {tag!r} {key[2]}", nbytes, device, zero=True)
            self.fixed[key] = blk.view
        assert blk.nbytes == int(nbytes), (tag, key, blk.nbytes, nbytes)
        return blk.view

    def poison(self) -> None:
        """every `get` interior holds the pattern again (and what selfsim left there is forgotten); `zeroed` buffers keep
        their content: their contract is that the ticket returns to 0"""
        for blk in self.blocks.values():
            blk.refill()
        self.selfsim_record = None

    def check(self):
        """asserts every guard of every buffer; -> {name: (declared bytes, high-water mark)} per `get` tag and size and per
        `zeroed` tag and key"""
        out = {}
        for (tag, _, nbytes), blk in self.blocks.items():
            blk.check()
            out[f"{tag}[{nbytes}]"] = (nbytes, blk.high_water())
        for (tag, _, key), blk in self.fixed_blocks.items():
            blk.check()
            out[f"{tag}{key}"] = (blk.nbytes, blk.high_water())
        return out


class Guard:
    """what `guarded` returns next to the tensor"""

    def __init__(self, block: Block, tensor: torch.Tensor, fill):
        self.block, self.tensor = block, tensor
        self.fill_bits = torch.full((1,), fill, dtype=tensor.dtype, device=tensor.device).view(torch.uint8)

    def check(self) -> None:
        self.block.check()

    def untouched(self, region: torch.Tensor = None) -> int:
        """the number of elements of the tensor (or of `region`, a view or an index of it) that still hold the fill, bit
        for bit"""
        t = self.tensor if region is None else region
        size = t.element_size()
        flat = t.contiguous().view(torch.uint8).reshape(-1, size)
        return int((flat == self.fill_bits).all(1).sum())


def guarded(shape, dtype, fill, device="cuda", name: str = "output"):
    """-> (tensor of `shape` and `dtype` filled with `fill`, its Guard): the tensor is the exact, 256-byte aligned interior
    of a guarded allocation of its own"""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    numel = 1
    for s in shape:
        numel *= s
    blk = Block(f"{name} {shape}", numel * torch.empty((), dtype=dtype).element_size(), device)
    t = blk.view.view(dtype).reshape(shape)
    t.fill_(fill)
    return t, Guard(blk, t, fill)
