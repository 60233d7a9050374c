"""run_strotss._resolve on the MI355X ("The driver"): through run() every validator is entered once per
run -- for a single image, and for a three-frame sequence with computed flows, two temporal offsets and tracked regions,
where the frame path used to enter them again for every frame (and the flow validators for every computed pair)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _temporal_long_ref as TL  # noqa: E402
import _temporal_ref as T  # noqa: E402
import test_resolve_cpu as RC  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(RC.ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")


def test_a_run_enters_every_validator_once(tmp_path, monkeypatch):
    from PIL import Image
    RS = RC.RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    counts = RC._counted(monkeypatch)
    RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "one.jpg"), "--max_size", "64", "--level", "1",
                                         "--max_iter", "2"]))
    assert os.path.exists(tmp_path / "one.jpg")
    assert counts == dict(dict.fromkeys(RC.VALIDATORS, 1), _temporal_frames=0)       # no sequence: no offsets asked for
    for v in counts:
        counts[v] = 0
    frames, flows, out = (str(tmp_path / n) for n in ("frames", "flows", "out"))
    paths, _ = TL.occluder_sequence(frames, flows, n_frames=3, offsets=(1, 2))      # 48 x 64 frames; the flows are computed
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    outs = RS.run(RS.build_parser().parse_args([frames, style, "-o", out, "--video", "--compute_flow", "--flow_match",
                                                "--flow_robust", "--temporal_frames", "1", "2", "--auto_masks", "2",
                                                "--track_masks", "--level", "1", "--max_iter", "2"]))
    assert len(outs) == 3 and len(os.listdir(out)) == 3
    assert counts == dict.fromkeys(RC.VALIDATORS, 1)                                 # once per run, not once per frame
