"""run_strotss._resolve without a GPU ("The driver"): the command line is resolved once -- every
validator entered once, the job holding what each returns -- the refusals come in the order and with the texts they always
had (tests/golden/cli_refusals.json: the first ValueError of run() before _resolve existed, for command lines with two
independent mistakes), and below _resolve nothing validates or asks whether a flag is there."""
import argparse
import ast
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import run_strotss as RS  # noqa: E402

VALIDATORS = ("_auto_masks_input", "_refine_masks_input", "_track_masks_input", "_scribble_masks_input",
              "_style_transport_input", "_palette_transport_input", "_pixel_prior_input", "_photo_term_input",
              "_auto_sample_input", "_sample_map_input", "_content_weight_input", "_preserve_color_input",
              "_photo_smooth_input", "_output_size_input", "_video_inputs", "_flow_match_radius", "_flow_robust",
              "_temporal_frames", "_style_inputs")
with open(os.path.join(ROOT, "tests", "golden", "cli_refusals.json")) as f:
    REFUSALS = json.load(f)


def _parse(*extra, content="c.jpg"):
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


def _counted(monkeypatch):
    """every validator wrapped on the module, so that the ones entered from inside another are counted too"""
    counts = dict.fromkeys(VALIDATORS, 0)

    def wrap(name, inner):
        def counted(*a, **k):
            counts[name] += 1
            return inner(*a, **k)
        return counted
    for name in VALIDATORS:
        monkeypatch.setattr(RS, name, wrap(name, getattr(RS, name)))
    return counts


@pytest.fixture
def lines(tmp_path, monkeypatch):
    """{name: namespace}: the default command line, and between them a member of every flag family"""
    from PIL import Image
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames = tmp_path / "frames"
    frames.mkdir()
    for t in (1, 2, 3):
        Image.new("RGB", (8, 6), (10 * t, 0, 0)).save(frames / f"f{t}.png")
    Image.new("L", (8, 6), 128).save(tmp_path / "map.png")
    return {
        "default": _parse(),
        "sequence": _parse("--video", "--compute_flow", "--flow_match", "--flow_robust", "--flow_outer", "2", "--save_flow", "d",
                           "--temporal_frames", "2", "1", "--temporal_weight", "10", "--temporal_init",
                           "--auto_masks", "3", "--track_masks", "--mask_inertia", "0.5", "--refine_masks", "--save_masks", "d",
                           "--style_transport", "sinkhorn", "--sinkhorn_log", "--palette_transport", "sliced",
                           "--detail_weight", "1", "--tv_weight", "2", "--photo_weight", "3", "--photo_radius", "2",
                           "--sample_map", "auto", "--sample_floor", "0.5", "--content_weight_map", "w.png",
                           "--preserve_color", "transfer", "--photo_smooth", "--smooth_radius", "3",
                           "--output_size", "full", "--upsample_mode", "guided", content=str(frames)),
        "scribbles": _parse("--content_scribbles", "a.png", "--style_scribbles", "b.png", "--scribble_iters", "7",
                            "--save_masks", "d", "--style_transport", "sliced", "--sliced_projections", "5",
                            "--sample_map", str(tmp_path / "map.png"), "--preserve_color", "transfer", "--transfer_iters", "3",
                            "--output_size", "512"),
        "blend": _parse("--style_mix", "t.jpg", "u.jpg", "--style_weights", "1", "0", "3", "--preserve_color", "luminance"),
        "masks": _parse("--content_mask", "cm.png", "--style_mask", "sm.png", "--strips"),
    }


def test_every_validator_is_entered_once(lines, monkeypatch):
    counts = _counted(monkeypatch)
    for name, ns in lines.items():
        for v in counts:
            counts[v] = 0
        RS._resolve(ns)
        want = dict.fromkeys(VALIDATORS, 1)
        want["_temporal_frames"] = int(ns.video)             # the offsets are a sequence's: _video_inputs asks only then
        assert counts == want, name


def test_the_job_holds_what_each_validator_returns(lines):
    for name, ns in lines.items():
        job = RS._resolve(ns)
        assert job.auto == RS._auto_masks_input(ns) and job.refine == RS._refine_masks_input(ns), name
        assert job.inertia == RS._track_masks_input(ns) and job.scribbles == RS._scribble_masks_input(ns), name
        assert job.engine_terms == dict(RS._style_transport_input(ns), **RS._palette_transport_input(ns)), name
        assert job.prior == RS._pixel_prior_input(ns) and job.photo == RS._photo_term_input(ns), name
        assert job.auto_sample == RS._auto_sample_input(ns) and job.sample_map == RS._sample_map_input(ns), name
        assert job.content_weight == RS._content_weight_input(ns), name
        assert job.preserve == RS._preserve_color_input(ns) and job.smooth == RS._photo_smooth_input(ns), name
        assert job.upsample == RS._output_size_input(ns) and job.styles == RS._style_inputs(ns), name
        assert job.match_radius == RS._flow_match_radius(ns) and job.robust == RS._flow_robust(ns), name
        if ns.video:
            assert (job.frames, job.temporal_weight) == RS._video_inputs(ns) and job.offsets == RS._temporal_frames(ns), name
        else:
            assert job.frames is None and job.offsets is None and job.temporal_weight is None, name
        if job.preserve == "transfer":
            assert job.transfer_iters == (RS.strotss.DEFAULT_TRANSFER_ITERS if ns.transfer_iters is None else ns.transfer_iters)
        again = RS._resolve(job)                             # a job is a namespace: resolving it again changes nothing
        assert vars(again) == vars(job), name
    job = RS._resolve(lines["sequence"])                     # spot values, so that the comparison above is not None == None
    assert job.auto == (3, "d") and job.refine == 0.1 and job.inertia == 0.5 and job.offsets == (1, 2)
    assert job.match_radius == 2 and job.robust == {"outer": 2} and job.temporal_weight == 10.0 and len(job.frames) == 3
    assert job.engine_terms["style_transport"] == "sinkhorn" and job.engine_terms["palette_transport"] == "sliced"
    assert job.photo == (3.0, 2, 1e-4) and job.transfer_iters == RS.strotss.DEFAULT_TRANSFER_ITERS
    assert RS._resolve(lines["blend"]).styles == (["s.jpg", "u.jpg"], [0.25, 0.75])
    assert RS._resolve(lines["scribbles"]).scribbles == ("a.png", "b.png", RS.strotss.SCRIBBLE_SIGMA, 7)


def test_a_partial_namespace_is_completed_with_the_parsers_defaults(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    given = argparse.Namespace(content_path="c.jpg", style_path="s.jpg", max_size=64, tv_weight=2.0)
    job, default = RS._resolve(given), _parse()
    for flag, value in vars(default).items():
        assert getattr(job, flag) == getattr(given, flag, value), flag
    assert job.prior == dict(detail=None, tv=2.0) and job.level == 4 and job.log_every == 10 and job.style_transport == "remd"
    assert vars(given) == dict(content_path="c.jpg", style_path="s.jpg", max_size=64, tv_weight=2.0)     # the caller's stays


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: " ".join(c["argv"]) + (f" WORLD_SIZE={c['world_size']}" if c["world_size"] else ""))
def test_of_two_wrong_flags_the_same_one_is_reported(case, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    if case["world_size"]:
        monkeypatch.setenv("WORLD_SIZE", str(case["world_size"]))
    for entry in (RS._resolve, RS.run):
        with pytest.raises(ValueError) as e:
            entry(_parse(*case["argv"], content="no_such_content.jpg"))
        assert str(e.value) == case["error"]


def test_the_recorded_refusals_cover_what_they_should():
    assert len(REFUSALS) >= 20
    texts = [c["error"] for c in REFUSALS]
    for what in ("--content_weight_map", "--sample_map", "--preserve_color", "--style_transport sliced",
                 "--style_transport sinkhorn", "--palette_transport sliced", "--detail_weight / --tv_weight", "--photo_weight",
                 "--photo_smooth", "--output_size", "--auto_masks", "--video"):
        assert f"{what} cannot be combined with --strips" in texts
        assert f"{what} runs on one GPU: not under torchrun with WORLD_SIZE > 1" in texts
    assert "scribbles cannot be combined with --strips" in texts
    assert "scribbles run on one GPU: not under torchrun with WORLD_SIZE > 1" in texts


def test_the_two_refusals_that_moved_come_before_any_image_is_opened(monkeypatch):
    """_style_inputs' refusals and the both-or-neither mask check used to be reached inside _stylise, after the VGG was built
    and the content decoded: with a content path that does not exist they are what run() reports now"""
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match=r"--style_weights takes 1 values \(style_path \+ 0 --style_mix images\), got 2"):
        RS.run(_parse("--style_weights", "1", "2", content="no_such_content.jpg"))
    with pytest.raises(ValueError) as e:
        RS.run(_parse("--content_mask", "cm.png", content="no_such_content.jpg"))
    assert str(e.value) == 'Either both content and style masks must be provided or neither.'
    with pytest.raises(ValueError) as e:                     # _style_inputs first, the mask pair after it
        RS.run(_parse("--style_mask", "sm.png", "--style_mix", "t.jpg", content="no_such_content.jpg"))
    assert str(e.value) == "style blending (--style_mix) cannot be combined with masks"


def test_below_resolve_nothing_validates_or_asks_for_a_flag():
    tree = ast.parse(inspect.getsource(RS))
    functions = [n for n in tree.body if isinstance(n, ast.FunctionDef)]
    resolve_line = next(f.lineno for f in functions if f.name == "_resolve")
    assert all(f.lineno < resolve_line for f in functions if f.name in VALIDATORS)
    called = lambda f: {c.func.id for c in ast.walk(f) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
    below = [f for f in functions if f.lineno > resolve_line]
    assert {"run", "run_video", "_stylise", "_region_masks", "_sample_map", "_recolour_styles", "_written_guides",
            "_tracked_masks", "_frame_at_result_size", "_computed_flows", "_flow_warp_for_frame", "_pairs_for_frame",
            "_temporal_targets_for_frame", "_optimise_scale", "_load_masks"} <= {f.name for f in below}
    for f in below:
        assert "getattr" not in called(f), f.name
    for f in functions:
        if f.name not in VALIDATORS + ("_resolve",):
            assert not called(f) & set(VALIDATORS), f.name
    assert called(next(f for f in functions if f.name == "run_video")) >= {"_resolve"}
