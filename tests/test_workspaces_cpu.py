"""nn._ops.Workspaces on host tensors: the grow-only scratch, the zeroed buffers of one layout, the
record of the content loss and the freeze, and that two instances share none of them.  No library is loaded."""
import pytest
import torch

from nn import _hip, _ops

CPU = torch.device("cpu")


def test_get_keeps_a_buffer_that_fits_and_replaces_one_that_does_not():
    ws = _ops.Workspaces()
    a = ws.get("selfsim", 1000, CPU)
    assert a.dtype == torch.uint8 and a.numel() == 1000
    assert ws.get("selfsim", 1000, CPU) is a and ws.get("selfsim", 10, CPU) is a
    b = ws.get("selfsim", 1001, CPU)
    assert b is not a and b.numel() == 1001 and ws.get("selfsim", 1000, CPU) is b
    assert ws.get("moment", 1, CPU).numel() == 256                        # the floor
    assert ws.get("moment", 1, CPU) is not b                              # one buffer per tag
    assert set(ws.bufs) == {("selfsim", "cpu"), ("moment", "cpu")} and ws.bufs[("selfsim", "cpu")] is b


def test_two_instances_share_no_buffer_and_no_record():
    one, two = _ops.Workspaces(), _ops.Workspaces()
    a, b = one.get("remd", 512, CPU), two.get("remd", 512, CPU)
    assert a is not b and a.data_ptr() != b.data_ptr()
    za, zb = one.zeroed("temporal", (4, 4), 64, CPU), two.zeroed("temporal", (4, 4), 64, CPU)
    assert za is not zb and za.data_ptr() != zb.data_ptr()
    assert one.bufs is not two.bufs and one.fixed is not two.fixed
    one.get("remd", 4096, CPU)                                            # growth in one ...
    assert two.get("remd", 512, CPU) is b                                 # ... leaves the other's buffer where it was
    assert _ops.workspaces is not one and isinstance(_ops.workspaces, _ops.Workspaces)


def test_zeroed_is_one_zero_filled_buffer_per_key():
    ws = _ops.Workspaces()
    a = ws.zeroed("color_stats", (48, 64), 4000, CPU)
    assert a.dtype == torch.uint8 and a.numel() == 4000 and not bool(a.any())
    assert ws.zeroed("color_stats", (48, 64), 4000, CPU) is a
    b = ws.zeroed("color_stats", (64, 48), 4000, CPU)                     # another shape of the same size: its own buffer
    c = ws.zeroed("detail_map", (48, 64), 4000, CPU)                      # another tag
    assert b is not a and c is not a and c is not b and not bool(b.any()) and not bool(c.any())
    a.fill_(7)                                                            # what a call leaves behind stays with its key
    assert bool((ws.zeroed("color_stats", (48, 64), 4000, CPU) == 7).all()) and not bool(b.any())
    assert not ws.bufs                                                    # kept apart from the scratch that tests fill


def test_freeze_refuses_growth_only():
    ws = _ops.Workspaces()
    a = ws.get("winograd", 1000, CPU)
    ws.freeze()
    assert ws.get("winograd", 1000, CPU) is a and ws.get("winograd", 1, CPU) is a      # a request that fits
    assert ws.get("conv_splitk", 5000, CPU).numel() == 5000                            # a tag never asked for before
    with pytest.raises(_hip.StrotssHipError) as err:
        ws.get("winograd", 1001, CPU)
    assert "winograd" in str(err.value) and "1000" in str(err.value) and "1001" in str(err.value)
    assert ws.get("winograd", 1000, CPU) is a                                          # nothing was reallocated
    with pytest.raises(_hip.StrotssHipError) as err:
        ws.get("conv_splitk", 5001, CPU)                                               # the new tag is held to its size too
    assert "conv_splitk" in str(err.value)
    assert ws.zeroed("tv", (8, 8), 64, CPU).numel() == 64                              # a zeroed buffer never grows anyway
    assert _ops.Workspaces().get("winograd", 1001, CPU).numel() == 1001                # another instance is not frozen


def test_the_selfsim_record_belongs_to_its_instance():
    one, two = _ops.Workspaces(), _ops.Workspaces()
    assert one.selfsim_record is None and two.selfsim_record is None
    rec = (one.get("selfsim", 256, CPU).data_ptr(), 256, 1234, 16, 32, 0)
    one.selfsim_record = rec
    assert one.selfsim_record == rec and two.selfsim_record is None and _ops.workspaces.selfsim_record != rec
