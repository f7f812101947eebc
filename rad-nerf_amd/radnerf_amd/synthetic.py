"""Seeded synthetic inputs of SURVEY.md §8(d) (numpy, so the CPU oracle and the
GPU path see bit-identical data):  rays seed 0, occupancy seed 1, jitter seed 2,
parameters seed 3 (module init), loss seeds seed 4."""
from types import SimpleNamespace

import numpy as np


def rays(n, scale=0.5, seed=0):
    """rays_o = R*u (u uniform on S^2, R = 3*scale), rays_d = normalize(p - rays_o),
    p ~ U([-0.8*scale, 0.8*scale]^3)."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (3.0 * scale * u).astype(np.float32)
    p = rng.uniform(-0.8 * scale, 0.8 * scale, size=(n, 3))
    d = p - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def bitfields(n_models, cascades, p=0.5, seed=1, grid_size=128):
    """Independent Bernoulli(p) occupancy per cell, per model and cascade."""
    rng = np.random.default_rng(seed)
    n_cells = cascades * grid_size ** 3
    occ = rng.random((n_models, n_cells)) < p
    return np.packbits(occ.reshape(n_models, -1, 8), axis=-1, bitorder="little").reshape(
        n_models, n_cells // 8)


def noise(n_models, n_rays, seed=2):
    return np.random.default_rng(seed).random((n_models, n_rays), dtype=np.float32)


def loss_seeds(n_rays, n_models, seed=4, std=1e-3):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, std, (n_rays, 3)).astype(np.float32),
            rng.normal(0, std, n_rays).astype(np.float32),
            rng.normal(0, std, (n_rays, n_models)).astype(np.float32))


def grid_params(n_entries, seed=3, amp=1e-1):
    """Hash-table values.  tcnn initialises U(-1e-4, 1e-4); parity tests use a
    larger amplitude so the field is far from trivial."""
    return np.random.default_rng(seed).uniform(-amp, amp, (n_entries, 2)).astype(np.float32)


def mlp_params(n_models, n_params, seed=5, scale=0.3):
    return np.random.default_rng(seed).uniform(-scale, scale, (n_models, n_params)).astype(
        np.float32)


# ---- cameras and whole scenes (torch is imported inside, the module itself needs numpy alone) ----
def ring_cameras(n_img, res, radius=1.5, half=0.3):
    """n_img cameras on a ring around the origin, looking at it (c2w columns
    right / up / forward): unit pixel directions (res * res, 3) of half-width
    `half` at unit depth, and poses (n_img, 3, 4)."""
    import torch
    u = torch.linspace(-half, half, res)
    y, x = torch.meshgrid(u, u, indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(res * res)], -1)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    ang = torch.arange(n_img) * (2 * np.pi / n_img) + 0.3
    pos = torch.stack([radius * torch.cos(ang), radius * torch.sin(ang),
                       0.4 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2)
    return dirs.contiguous(), poses.contiguous()


class Scene(SimpleNamespace):
    """what a scene builder returns, by name (m model, g gate, bits, ...)"""


def set_bitfields(model, bits):
    """density_bitfield_i <- bits[i] for every sub-NeRF (an NGP has one);
    bits is (K, bytes), a numpy array or a tensor."""
    import torch
    with torch.no_grad():
        for i in range(model.size):
            # (torch.tensor copies, so a read-only array will do)
            b = bits[i] if torch.is_tensor(bits[i]) else torch.tensor(bits[i])
            getattr(model, f"density_bitfield_{i}").copy_(b)


def parity_scene(K, B=None, scale=0.5, p=0.5, gate_type="ray", rough_grid=True, device=None):
    """The tests' recipe: module seeds 3 / 2, then every parameter overwritten
    from this file's tables (grid unless rough_grid=False: the module's own
    init), Bernoulli(p) occupancy.  With B also the numpy rays, jitter and
    loss seeds of one batch.  -> Scene(m, g, bits, o, d, noise, seeds)."""
    import torch
    from . import layout as LY
    from .networks import MNGP, Ray_Gate
    m, g = MNGP(scale, size=K, seed=3), Ray_Gate(K, type=gate_type, seed=2)
    with torch.no_grad():
        if rough_grid:
            m.xyz_encoder.params.copy_(torch.from_numpy(grid_params(m.xyz_encoder.n_entries)).view(-1))
        m.mlp_params.copy_(torch.from_numpy(mlp_params(K, LY.FIELD_PARAMS)))
        g.params.copy_(torch.from_numpy(mlp_params(1, LY.gate_params(K), seed=6)[0]))
    bits = bitfields(K, m.cascades, p)
    set_bitfields(m, bits)
    sc = Scene(m=m.to(device), g=g.to(device), bits=bits, o=None, d=None, noise=None, seeds=None)
    if B is not None:
        sc.o, sc.d = rays(B, scale)
        sc.noise, sc.seeds = noise(K, B), loss_seeds(B, K)
    return sc


def bench_scene(K, B, scale, device, p=0.5):
    """bench.py's and the tools' recipe: module seeds 3 / 4 with the modules'
    own initial parameters (an NGP when K == 1), occupancy seed 1, rays seed 0,
    jitter seed 2, loss seeds seed 4, all on `device`; exp_step_factor and
    background by scale; zeroed gradient buffers.
    -> Scene(m, g, bits, o, d, noise, seeds, esf, bg, grid_grad, mlp_grad, gate_grad)."""
    import torch
    from .networks import MNGP, NGP, Ray_Gate
    m = (NGP(scale, seed=3) if K == 1 else MNGP(scale, size=K, seed=3)).to(device)
    g = Ray_Gate(K, seed=4).to(device)
    bits = bitfields(K, m.cascades, p=p, seed=1)
    set_bitfields(m, bits)
    to = lambda a: torch.from_numpy(a).to(device)
    o, d = (to(a) for a in rays(B, scale, seed=0))
    esf = 1 / 256 if scale > 0.5 else 0.0
    return Scene(m=m, g=g, bits=bits, o=o, d=d, noise=to(noise(K, B, seed=2)),
                 seeds=tuple(to(s) for s in loss_seeds(B, K, seed=4)), esf=esf,
                 bg=torch.ones(3, device=device) if esf == 0 else torch.zeros(3, device=device),
                 grid_grad=torch.zeros_like(m.xyz_encoder.params),
                 mlp_grad=torch.zeros_like(m.mlp_params), gate_grad=torch.zeros_like(g.params))
