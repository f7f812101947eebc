"""The two scene builders of radnerf_amd/synthetic.py against their recipes
spelled out from the module's primitives (CPU), and set_bitfields."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from radnerf_amd import layout as LY
from radnerf_amd import synthetic as S
from radnerf_amd.networks import MNGP, NGP, Ray_Gate

K, B, SCALE = 2, 64, 0.5


def _bitfields_of(m):
    return np.stack([getattr(m, f"density_bitfield_{i}").numpy() for i in range(m.size)])


def _same(a, b):
    """two scenes: every parameter, buffer and array equal"""
    for x, y in ((a.m, b.m), (a.g, b.g)):
        sx, sy = x.state_dict(), y.state_dict()
        assert sx.keys() == sy.keys()
        assert all(torch.equal(sx[k], sy[k]) for k in sx)
    assert np.array_equal(a.bits, b.bits)
    flat = lambda sc: [sc.o, sc.d, sc.noise, *sc.seeds]
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("gate_type,rough_grid,p", [("ray", True, 0.5), ("image", False, 0.3)])
def test_parity_scene_is_its_recipe(gate_type, rough_grid, p):
    sc = S.parity_scene(K, B, scale=SCALE, p=p, gate_type=gate_type, rough_grid=rough_grid,
                        device="cpu")
    m, g = MNGP(SCALE, size=K, seed=3), Ray_Gate(K, type=gate_type, seed=2)
    own_grid = m.xyz_encoder.params.detach().clone()
    want_grid = torch.from_numpy(S.grid_params(m.xyz_encoder.n_entries)).view(-1) \
        if rough_grid else own_grid
    assert torch.equal(sc.m.xyz_encoder.params, want_grid)
    assert rough_grid or not torch.equal(own_grid, torch.from_numpy(
        S.grid_params(m.xyz_encoder.n_entries)).view(-1))
    assert torch.equal(sc.m.mlp_params, torch.from_numpy(S.mlp_params(K, LY.FIELD_PARAMS)))
    assert torch.equal(sc.g.params,
                       torch.from_numpy(S.mlp_params(1, LY.gate_params(K), seed=6)[0]))
    assert sc.g.state_dict().keys() == g.state_dict().keys()
    bits = S.bitfields(K, m.cascades, p)
    assert np.array_equal(sc.bits, bits) and np.array_equal(_bitfields_of(sc.m), bits)
    o, d = S.rays(B, SCALE)
    assert np.array_equal(sc.o, o) and np.array_equal(sc.d, d)
    assert np.array_equal(sc.noise, S.noise(K, B))
    assert all(np.array_equal(a, b) for a, b in zip(sc.seeds, S.loss_seeds(B, K)))
    # every other buffer is the module's own
    own = m.state_dict()
    for k, v in sc.m.state_dict().items():
        if "bitfield" not in k and k not in ("xyz_encoder.params", "mlp_params"):
            assert torch.equal(v, own[k]), k
    _same(sc, S.parity_scene(K, B, scale=SCALE, p=p, gate_type=gate_type, rough_grid=rough_grid,
                             device="cpu"))


def test_parity_scene_without_a_batch():
    sc = S.parity_scene(K, device="cpu")
    assert sc.o is sc.d is sc.noise is sc.seeds is None
    assert np.array_equal(_bitfields_of(sc.m), S.bitfields(K, sc.m.cascades, 0.5))


@pytest.mark.parametrize("k", [K, 1])
def test_bench_scene_is_its_recipe(k):
    sc = S.bench_scene(k, B, SCALE, "cpu")
    m = NGP(SCALE, seed=3) if k == 1 else MNGP(SCALE, size=k, seed=3)
    g = Ray_Gate(k, seed=4)
    assert type(sc.m) is type(m)
    bits = S.bitfields(k, m.cascades, p=0.5, seed=1)
    S.set_bitfields(m, bits)
    for got, want in ((sc.m, m), (sc.g, g)):
        sd = want.state_dict()
        assert got.state_dict().keys() == sd.keys()
        assert all(torch.equal(v, sd[n]) for n, v in got.state_dict().items())
    assert np.array_equal(sc.bits, bits)
    o, d = S.rays(B, SCALE, seed=0)
    assert np.array_equal(sc.o.numpy(), o) and np.array_equal(sc.d.numpy(), d)
    assert np.array_equal(sc.noise.numpy(), S.noise(k, B, seed=2))
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(sc.seeds, S.loss_seeds(B, k, seed=4)))
    assert sc.esf == 0.0 and torch.equal(sc.bg, torch.ones(3))
    for grad, p in ((sc.grid_grad, m.xyz_encoder.params), (sc.mlp_grad, m.mlp_params),
                    (sc.gate_grad, g.params)):
        assert grad.shape == p.shape and grad.dtype == p.dtype and not grad.any()
    _same(sc, S.bench_scene(k, B, SCALE, "cpu"))


def test_bench_scene_background_and_step_by_scale():
    sc = S.bench_scene(K, 8, 16.0, "cpu")
    assert sc.esf == 1 / 256 and torch.equal(sc.bg, torch.zeros(3))
    assert np.array_equal(sc.o.numpy(), S.rays(8, 16.0, seed=0)[0])


@pytest.mark.parametrize("make", [lambda: MNGP(SCALE, size=3, seed=0), lambda: NGP(SCALE, seed=0)])
def test_set_bitfields_round_trips(make):
    m = make()
    bits = S.bitfields(m.size, m.cascades, p=0.4, seed=9)
    bits.setflags(write=False)
    S.set_bitfields(m, bits)
    assert np.array_equal(_bitfields_of(m), bits)
    flipped = torch.from_numpy(~bits)
    S.set_bitfields(m, flipped)
    assert torch.equal(torch.stack([getattr(m, f"density_bitfield_{i}") for i in range(m.size)]),
                       flipped)
    assert not any(p.grad is not None for p in m.parameters())


def test_synthetic_imports_without_torch():
    code = ("import sys; import radnerf_amd.synthetic as S; "
            "assert 'torch' not in sys.modules, 'torch imported'; S.rays(4)")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
