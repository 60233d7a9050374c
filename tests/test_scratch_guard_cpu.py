"""CPU: the guard bands of tests/_scratch_guard.py have teeth.  On CPU tensors: buffers are exact and aligned, a repeated
size is the same storage, freeze refuses growth, check() passes on an untouched buffer and after writes to the first and
last interior byte, and fails -- naming the tag and the offset -- after ONE byte just in front of the interior, just behind
it or at the far end of a guard; zeroed buffers survive poison().  tests/test_hip_scratch_contracts.py relies on exactly
these checks on the GPU, where no under-sized request is ever run on purpose."""
import numpy as np
import pytest
import torch

import _scratch_guard as SG

CPU = "cpu"
SIZES = (1, 3, 255, 256, 257, 4099, 5 * (1 << 20) + 2)


def _pattern_ok(t):
    return bool((t.view(torch.int32) == SG.PATTERN).all())


@pytest.mark.parametrize("nbytes", SIZES)
def test_buffers_are_exact_aligned_and_patterned(nbytes):
    ws = SG.GuardedWorkspaces()
    b = ws.get("t", nbytes, CPU)
    blk = ws.blocks[("t", CPU, nbytes)]
    assert b.dtype == torch.uint8 and b.numel() == nbytes and b.data_ptr() % SG.ALIGN == 0
    assert blk.guard >= SG.MIN_GUARD and 4 * blk.guard >= nbytes
    assert blk.off >= blk.guard and blk.backing.numel() - (blk.off + nbytes) >= blk.guard          # both guards are whole
    assert b.data_ptr() == blk.backing.data_ptr() + blk.off
    assert _pattern_ok(blk.backing[:blk.backing.numel() // 4 * 4])                                  # guards AND fresh interior
    assert ws.check() == {f"t[{nbytes}]": (nbytes, -1)}
    z = ws.zeroed("z", (3, 5), nbytes, CPU)
    assert z.numel() == nbytes and z.data_ptr() % SG.ALIGN == 0 and not z.any()
    out = ws.check()
    assert out["z(3, 5)"] == (nbytes, -1) and len(out) == 2


def test_same_size_same_storage_another_size_an_exact_new_one():
    ws = SG.GuardedWorkspaces()
    a = ws.get("t", 1000, CPU)
    assert ws.get("t", 1000, CPU) is a
    other = ws.get("u", 1000, CPU)
    assert other.data_ptr() != a.data_ptr()
    b = ws.get("t", 400, CPU)                               # smaller: the product would hand back the 1000 bytes
    assert b.numel() == 400 and b.data_ptr() != a.data_ptr() and ws.bufs[("t", CPU)] is b
    c = ws.get("t", 1000, CPU)                              # a size seen before: its storage again (a graph may point there)
    assert c.data_ptr() == a.data_ptr() and c.numel() == 1000
    assert ws.zeroed("z", (1, 2), 64, CPU) is ws.zeroed("z", (1, 2), 64, CPU)
    assert ws.zeroed("z", (2, 1), 64, CPU).data_ptr() != ws.zeroed("z", (1, 2), 64, CPU).data_ptr()
    assert sorted(ws.check()) == ["t[1000]", "t[400]", "u[1000]", "z(1, 2)", "z(2, 1)"]


def test_a_request_of_another_size_checks_the_buffer_it_leaves():
    ws = SG.GuardedWorkspaces()
    a = ws.get("t", 1000, CPU)
    blk = ws.blocks[("t", CPU, 1000)]
    blk.backing[blk.off + 1000] ^= 1
    with pytest.raises(AssertionError, match=r"workspace 't' \(1000 bytes\).*offset 1000 "):
        ws.get("t", 2000, CPU)
    assert a.numel() == 1000


def test_freeze_refuses_growth_as_the_base_class_does():
    from nn import _hip
    ws = SG.GuardedWorkspaces()
    ws.get("t", 1000, CPU)
    ws.freeze()
    assert ws.frozen
    assert ws.get("t", 1000, CPU).numel() == 1000           # fits
    assert ws.get("t", 300, CPU).numel() == 300             # fits (the product serves it from the 1000 bytes)
    assert ws.get("new", 5000, CPU).numel() == 5000         # a new tag is served as before
    with pytest.raises(_hip.StrotssHipError, match="frozen"):
        ws.get("t", 1001, CPU)


@pytest.mark.parametrize("nbytes", SIZES)
def test_check_passes_on_interior_writes_and_reports_the_high_water_mark(nbytes):
    ws = SG.GuardedWorkspaces()
    b = ws.get("t", nbytes, CPU)
    b[0] ^= 0xFF
    assert ws.check()["t[%d]" % nbytes] == (nbytes, 0)
    b[nbytes - 1] ^= 0x0F
    assert ws.check()["t[%d]" % nbytes] == (nbytes, nbytes - 1)
    ws.poison()
    assert ws.check()["t[%d]" % nbytes] == (nbytes, -1)
    t, g = SG.guarded((3, 5, 7), torch.float32, float("nan"), CPU)
    assert t.shape == (3, 5, 7) and t.data_ptr() % SG.ALIGN == 0 and g.untouched() == 105
    t[0, 0, 0], t[2, 4, 6] = 1.0, float("nan")              # another NaN than the fill's?  the same bits: still untouched
    g.check()
    assert g.untouched() == 104 and g.untouched(t[2]) == 35 and g.untouched(t[0]) == 34


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("where", ["just_before", "just_behind", "far_before", "far_behind"])
def test_check_fails_on_one_guard_byte_and_names_tag_and_offset(nbytes, where):
    ws = SG.GuardedWorkspaces()
    ws.get("other", 64, CPU)
    ws.get("victim", nbytes, CPU)
    blk = ws.blocks[("victim", CPU, nbytes)]
    at = {"just_before": blk.off - 1, "just_behind": blk.off + nbytes, "far_before": 0,
          "far_behind": blk.backing.numel() - 1}[where]
    blk.backing[at] ^= 0x01                                  # one bit of one byte
    with pytest.raises(AssertionError) as e:
        ws.check()
    msg = str(e.value)
    assert "workspace 'victim'" in msg and f"({nbytes} bytes)" in msg and "1 guard bytes" in msg
    assert f"offset {at - blk.off} " in msg, msg
    blk.backing[at] ^= 0x01
    ws.check()


@pytest.mark.parametrize("dtype,fill", [(torch.float32, float("nan")), (torch.uint8, 9), (torch.int32, -5), (torch.float64, -7.0)])
def test_guarded_tensors_fail_the_same_way(dtype, fill):
    t, g = SG.guarded((5, 3), dtype, fill, CPU, name="pool_code")
    size = t.element_size()
    assert t.dtype == dtype and g.untouched() == 15 and g.block.nbytes == 15 * size
    g.check()
    for at in (g.block.off - 1, g.block.off + 15 * size, g.block.backing.numel() - 1):
        g.block.backing[at] ^= 0x80
        with pytest.raises(AssertionError, match=rf"pool_code \(5, 3\).*offset {at - g.block.off} "):
            g.check()
        g.block.backing[at] ^= 0x80
    g.check()
    t.view(-1)[14] = 1
    assert g.untouched() == 14


def test_zeroed_survives_poison_and_get_does_not():
    ws = SG.GuardedWorkspaces()
    z = ws.zeroed("ticket", (8, 8), 48, CPU)
    b = ws.get("t", 48, CPU)
    z[4:8] = torch.tensor([1, 2, 3, 4], dtype=torch.uint8)
    b[:] = 0
    ws.selfsim_record = ("something",)
    ws.poison()
    assert z[4:8].tolist() == [1, 2, 3, 4] and not z[:4].any() and not z[8:].any()
    assert np.array_equal(b.numpy().view(np.int32), np.full(12, SG.PATTERN, np.int32))
    assert ws.selfsim_record is None
    assert ws.check() == {"t[48]": (48, -1), "ticket(8, 8)": (48, 7)}
    blk = ws.fixed_blocks[("ticket", CPU, (8, 8))]
    blk.backing[blk.off + 48] = 0
    with pytest.raises(AssertionError, match=r"zeroed workspace 'ticket' \(8, 8\) \(48 bytes\).*offset 48 "):
        ws.check()
