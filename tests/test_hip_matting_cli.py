"""--photo_weight end to end on the MI355X, at --max_size 64 --level 1 --max_iter 30, deterministic, on
tests/golden's images: E_m, L_photo of the written result against the content from the float64 restatement (r = 1,
eps = 1e-4), with the flag off and at SUGGESTED_PHOTO_WEIGHT -- the bound is the geometric mean of the measured ratio and 1;
the run without the flag writes the bytes it wrote before the flag existed, whatever the namespace looks like; and
--video --compute_flow runs with the term and lowers E_m in every frame."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _matting_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SUGGESTED_PHOTO_WEIGHT = 10.0      # DESIGN.md section 33's suggested starting value
PHOTO_RATIO = 0.234                # E_m(on) < ratio * E_m(off): measured 0.000415 / 0.0075922 = 0.0547, sqrt(0.0547 * 1)
# sha256 of the JPEG this run wrote before the flags existed (recorded on an MI355X from the commit before them)
PLAIN_JPEG_SHA256 = "38c675789663aa5057e67757594fe9e966aaeb80aaed8ae764125de37aa4aab9"


def _parse(tmp_path, name, *extra, ext="png"):
    import run_strotss as RS
    out = str(tmp_path / f"{name}.{ext}")
    return out, RS.build_parser().parse_args([os.path.join(GOLD, "content_im.jpg"), os.path.join(GOLD, "style_im.jpg"),
                                              "--max_size", "64", "--level", "1", "--max_iter", "30", "-o", out] + list(extra))


def _e_m(path, content):
    from PIL import Image
    result = np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0
    assert result.shape == content.shape
    return MR.value_grad(result, content, 1, 1e-4)[0]


def test_suggested_weight_lowers_the_matting_energy(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    import run_strotss as RS
    e = []
    for name, extra in (("off", ()), ("on", ("--photo_weight", f"{SUGGESTED_PHOTO_WEIGHT:g}"))):
        out, args = _parse(tmp_path, name, *extra)
        RS.run(args)
        content = RS._frame_at_result_size(RS._resolve(args), args.content_path).cpu().numpy().astype(np.float64)
        e.append(_e_m(out, content))
    print(f"MEASURE end to end: E_m off {e[0]:.6e} on {e[1]:.6e} ratio {e[1] / e[0]:.4f} (bound {PHOTO_RATIO})")
    assert e[1] < PHOTO_RATIO * e[0], e
    # the other flags reach the term: another radius and eps write another image
    out2, args2 = _parse(tmp_path, "r2", "--photo_weight", f"{SUGGESTED_PHOTO_WEIGHT:g}", "--photo_radius", "2", "--photo_eps", "0.01")
    RS.run(args2)
    with open(out2, "rb") as a, open(str(tmp_path / "on.png"), "rb") as b:
        assert a.read() != b.read()


def test_without_the_flag_the_written_bytes_are_the_earlier_ones(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    import run_strotss as RS
    out, args = _parse(tmp_path, "plain", ext="jpg")
    assert args.photo_weight is None
    RS.run(args)
    with open(out, "rb") as f:
        plain = f.read()
    print(f"MEASURE plain run: sha256 {hashlib.sha256(plain).hexdigest()}")
    assert hashlib.sha256(plain).hexdigest() == PLAIN_JPEG_SHA256
    out2, bare = _parse(tmp_path, "bare", ext="jpg")
    for k in ("photo_weight", "photo_radius", "photo_eps"):              # a namespace from before the flags existed
        delattr(bare, k)
    RS.run(bare)
    with open(out2, "rb") as f:
        assert f.read() == plain


def test_video_with_computed_flow_runs_with_the_term(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    import run_strotss as RS
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three shifted crops of one texture
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    energies = {}
    for name, extra in (("off", []), ("on", ["--photo_weight", f"{SUGGESTED_PHOTO_WEIGHT:g}"])):
        out = tmp_path / name
        RS.run(RS.build_parser().parse_args([frames, style, "--video", "--compute_flow", "-o", str(out), "--max_size", "64",
                                             "--level", "1", "--max_iter", "30"] + extra))
        energies[name] = []
        for q in paths:
            content = np.asarray(Image.open(q).convert("RGB"), dtype=np.float64) / 255.0
            energies[name].append(_e_m(str(out / (os.path.splitext(os.path.basename(q))[0] + ".jpg")), content))
    print(f"MEASURE video: E_m per frame off {energies['off']} on {energies['on']}")
    assert len(energies["on"]) == 3 and all(on < off for on, off in zip(energies["on"], energies["off"]))
