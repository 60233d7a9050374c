"""GPU: the F4_x3_gemm_128 route with V as f32 split in the GEMM's registers (STROTSS_X3_CONV_F32A=1, the default) computes
bit for bit what the x3-panel form (STROTSS_X3_CONV_F32A=0) computes.  The library reads the switch once per process, so
each setting runs in a child process that prints a digest of every output; the parent compares the two.

Cases: every layer routed to F4_x3_gemm_128 or F4_x3_gemm_64 at 512 and 1024 px (VGG16, forward and data-gradient), two
F4_x3_gemm_128 shapes whose tile count is not a multiple of 128, and one input seeded with special values (+-0, subnormals,
+-FLT_MAX, values exact in bf16) that reach V as they are and as small multiples, so the split in registers meets them
where split3 meets them in the panel producer.  Forward: the activation, the pooled copy, its argmax codes and the sign
words.  Data-gradient: plain, masked by sign words, and accumulating.  Then two short bench.py runs dump identical files."""
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import _route_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X3_ROUTES = ("F4_x3_gemm_128", "F4_x3_gemm_64")
SPECIAL = "special"          # case tag: the input of F4_x3_gemm_128's block3 shape seeded with special values


def _cases():
    """(route, direction, h, w, cin, cout[, tag]) of every x3 layer at 512 / 1024 px plus the ragged and special cases."""
    M = RC._model()
    out = []
    for px in (512, 1024):
        h = w = px
        for it in M.vgg_config("16"):
            if it == "pool":
                h, w = h // 2, w // 2
                continue
            _, cin, cout = it
            for direction, (ci, co) in (("fwd", (cin, cout)), ("dgrad", (cin, cout))):
                r = M.conv_route(h, w, ci, co, dgrad=direction == "dgrad")
                c = (r, direction, h, w, ci, co)
                if r in X3_ROUTES and c not in out:
                    out.append(c)
    # 63 x 63 = 3969 and 31 x 31 = 961 tiles: the last 128-row tile of every position is partial
    for h, cin, cout in ((250, 256, 256), (122, 512, 512)):
        for direction in ("fwd", "dgrad"):
            out.append((M.conv_route(h, h, cin, cout, dgrad=direction == "dgrad"), direction, h, h, cin, cout))
    out.append(("F4_x3_gemm_128", "fwd", 256, 256, 256, 256, SPECIAL))
    out.append(("F4_x3_gemm_128", "dgrad", 256, 256, 256, 256, SPECIAL))
    return out


def _special_values():
    f = np.float32
    fmax = np.finfo(f).max
    v = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, float(np.finfo(f).tiny), fmax, -fmax, fmax / 64, 1.5, -0.15625, 3.0,
         2.0 ** -126, 65280.0, 1.0 + 2.0 ** -7, float(f(1.0) + np.finfo(f).eps), -1e-30, 123.456, -7.777e7]
    return torch.tensor(np.array(v, dtype=f))


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:32]


def _run_case(case):
    """Digests of every output the case's layer writes, under this process's switch."""
    route, direction, h, w, cin, cout = case[:6]
    special = len(case) > 6
    M = RC._model()
    from nn import _ops as ops
    assert M.conv_route(h, w, cin, cout, dgrad=direction == "dgrad") == route, (case, "drifted")
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(case).encode()))
    ci_x = cin if direction == "fwd" else cout          # channels of the layer's transformed input
    x = torch.relu(torch.randn(1, h, w, ci_x, generator=g, device="cuda"))
    if special:
        # special values at pixels (4 ty + 4, 4 tx + 4): d[5][5] of tile (ty, tx) -> V = x, and d[1][1] of tile
        # (ty + 1, tx + 1) -> V = 16 x, 20 x, 25 x, ...; random sign flips elsewhere so that V has both signs
        x = x * torch.where(torch.rand(x.shape, generator=g, device="cuda") < 0.5, -1.0, 1.0)
        sv = _special_values().cuda()
        k = torch.arange(sv.numel(), device="cuda")
        for j in range(8):
            ys, xs, cs = 4 + 4 * (k + 5 * j), 4 + 4 * ((3 * k + j) % 60), (k * 13 + j * 31) % ci_x
            x[0, ys % (h - 4), xs, cs] = sv
    wt = torch.randn(3, 3, cin, cout, generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    res = {}
    if direction == "fwd":
        b = torch.randn(cout, generator=g, device="cuda") * 0.1
        u = ops.winograd_weights(wt.permute(3, 2, 0, 1), 4)
        out = torch.full((1, h, w, cout), -7.0, device="cuda")
        pool = torch.full((1, h // 2, w // 2, cout), -1.0, device="cuda")
        code = torch.full((1, h // 2, w // 2, cout), 9, dtype=torch.uint8, device="cuda")
        bits = ops.relu_bits_buffer(h, w, cout, "cuda").zero_()
        ops.conv3x3_winograd_fwd(x, u, b, out=out, pool_out=pool, pool_code=code, relu_bits_out=bits)
        res.update(out=_digest(out), pool_out=_digest(pool), pool_code=_digest(code), relu_bits=_digest(bits))
    else:
        u = ops.winograd_weights(wt.flip(0, 1).permute(2, 3, 0, 1), 4)
        act = torch.relu(torch.randn(1, h, w, cin, generator=g, device="cuda"))
        act_bits = ops.relu_bits(act)
        gin = ops.conv3x3_winograd_dgrad(x, u, cin, out=torch.full((1, h, w, cin), -7.0, device="cuda"))
        masked = ops.conv3x3_winograd_dgrad(x, u, cin, relu_bits=act_bits, out=torch.full((1, h, w, cin), -7.0, device="cuda"))
        pre = torch.randn(1, h, w, cin, generator=g, device="cuda")
        acc = ops.conv3x3_winograd_dgrad(x, u, cin, relu_bits=act_bits, out=pre, accumulate=True)
        res.update(dgrad=_digest(gin), dgrad_masked=_digest(masked), dgrad_accumulate=_digest(acc))
    torch.cuda.synchronize()
    return res


def _child(switch, *args, timeout=900):
    env = dict(os.environ, STROTSS_X3_CONV_F32A=str(switch))
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), env=env, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT)


def test_case_list_covers_both_x3_routes_and_ragged_tiles():
    cases = _cases()
    routes = {c[0] for c in cases}
    assert routes == set(X3_ROUTES), routes
    ragged = [c for c in cases if c[0] == "F4_x3_gemm_128" and (((c[2] + 3) // 4) * ((c[3] + 3) // 4)) % 128]
    assert {c[1] for c in ragged} == {"fwd", "dgrad"}, ragged


def test_f32_operand_matches_panels_bitwise():
    digests = []
    for switch in (0, 1):
        out = _child(switch, "cases")
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
        digests.append(json.loads(out.stdout.strip().splitlines()[-1]))
    assert list(digests[0]) == list(digests[1]) and len(digests[0]) == len(_cases())
    bad = [(k, q) for k in digests[0] for q in digests[0][k] if digests[0][k][q] != digests[1][k][q]]
    assert not bad, bad


def test_bench_dumps_identical_under_both_settings(tmp_path):
    dumps = []
    for switch in (0, 1):
        d = tmp_path / f"f32a{switch}"
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        env["STROTSS_X3_CONV_F32A"] = str(switch)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
                              "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        files = sorted(os.listdir(d))
        assert files, "no dump"
        dumps.append({f: np.load(d / f) for f in files})
    assert list(dumps[0]) == list(dumps[1])
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name


if __name__ == "__main__":          # child of the tests above: one setting of STROTSS_X3_CONV_F32A
    assert sys.argv[1] == "cases"
    print(json.dumps({repr(c): _run_case(c) for c in _cases()}))
