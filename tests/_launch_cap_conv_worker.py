"""Child process of tests/test_hip_launch_caps.py: the convolution rows of tests/_launch_cap_cases.py under one switch group
(`python _launch_cap_conv_worker.py GROUP`; the library reads its switches once per process).  Per case: integer data of the
exact family (tests/_exact_cases.py: int_params, 576 k with sparse +-1) made on the device, the library's route asserted, the
forward Winograd convolution into a NaN pre-fill, every element finite, and the SAMPLED tile rows bit for bit against the plain
float64 convolution of those rows (conv64 on the rows and one more on each side), after conditions 2 .. 5 on the same rows.
Prints one JSON line: {case: [figures, failures]}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import _exact_cases as E
import _launch_cap_cases as L

DEV = "cuda"


def device_problem(name):
    """E.make_int_problem's data law with the activation drawn on the device (270 M values)"""
    group, tile, (h, w, cin, cout), _, _ = L.CONV_CASES[name]
    route = {2: "F2_gemm_f32", 4: "F4_x3_gemm_128" if group != "f32_gemms" and cout >= 256 else "F4_gemm_f32"}[tile]
    p = E.Problem(name, route, "fwd", h, w, cin, cout)
    amax, density = E.int_params(route, p.K)
    g = torch.Generator(device=DEV).manual_seed(sum(map(ord, name)))
    v = torch.randint(1, amax + 1, (1, h, w, p.K), generator=g, device=DEV, dtype=torch.int16)
    p.a = (v * (torch.rand((1, h, w, p.K), generator=g, device=DEV) < 0.5)).float()
    gk = E._gen(name + ":k")
    sign = torch.where(torch.rand((3, 3, p.K, p.N), generator=gk) < 0.5, -1.0, 1.0)
    p.k_eff = (sign * (torch.rand((3, 3, p.K, p.N), generator=gk) < density)).to(DEV)
    p.bias = torch.randint(-E.BIAS_MAX, E.BIAS_MAX + 1, (cout,), generator=E._gen(name + ":b")).float().to(DEV)
    return p


def rows_reference(p, name):
    """float64 pre-activation of the sampled image rows (rows, w, N): conv64 per tile row on its rows and one beyond each side"""
    _, tile, (h, w, _, _), _, _ = L.CONV_CASES[name]
    k = 576.0 * p.k_eff
    out = []
    for ty in L.conv_tile_rows(name):
        y0, y1 = ty * tile, ty * tile + tile
        a0, a1 = max(y0 - 1, 0), min(y1 + 1, h)
        band = E.conv64(p.a[:, a0:a1], k)[0]                     # zero padding at a cut is wrong only in the band's outer rows
        pad = torch.zeros(tile, w, p.N, dtype=torch.float64, device=DEV)
        take = min(y1, h) - y0
        pad[:take] = band[y0 - a0:y0 - a0 + take]
        out.append(pad)
    return torch.cat(out) + p.bias.double()


def run_case(name):
    from nn import _hip, _ops
    group, tile, (h, w, cin, cout), which, want_route = L.CONV_CASES[name]
    p = device_problem(name)
    u = _ops.winograd_weights(p.wt.permute(3, 2, 0, 1), tile)
    want_u = E.exact_u(p.k_eff, tile).reshape((tile + 2) ** 2, p.K, p.N).transpose(1, 2)
    assert torch.equal(u.double(), want_u), (name, "condition 1")
    if tile == 4:
        packed = int(_ops.winograd_packed_wanted(36, cout, cin))
        x3 = int(_ops.winograd_x3(u, h, w) is not None)
        route = _hip.lib().strotss_conv3x3_winograd_route(h, w, cin, cout, 4, packed, x3)
        assert route == want_route, (name, "route", route, want_route)
    rows = L.conv_tile_rows(name)
    fig, _, _ = E.winograd_conditions(p, rows=rows)
    E.assert_winograd_conditions(fig, name)
    pre = rows_reference(p, name)
    y, inside = L.conv_image_rows(name)
    E.assert_nontrivial(pre[torch.as_tensor(inside, device=DEV)], name)
    out = torch.full((1, h, w, cout), float("nan"), device=DEV)
    _ops.conv3x3_winograd_fwd(p.a, u, p.bias, out=out)
    torch.cuda.synchronize()
    unwritten = int((~torch.isfinite(out)).sum())
    got = out[0][torch.as_tensor(np.minimum(y, h - 1), device=DEV)].cpu().numpy()
    figures, bad = L.conv_judge(name, got, torch.relu(pre).cpu().numpy(), unwritten)
    figures.update({k: round(v, 4) if isinstance(v, float) else v for k, v in fig.items()})
    del out, p, u
    torch.cuda.empty_cache()
    return figures, bad


if __name__ == "__main__":
    group = sys.argv[1]
    assert all(os.environ.get(k) == v for k, v in L.CONV_GROUPS[group].items()), "run with the group's environment"
    print(json.dumps({name: run_case(name) for name, c in L.CONV_CASES.items() if c[0] == group}))
