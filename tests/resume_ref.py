"""The training set-up of the resume tests (tests/test_gpu_resume.py,
tests/resume_dp_worker.py), restated from tests/test_gpu_deterministic.py:
four 32 x 32 images of the analytic sphere, cameras on a ring, 512 rays,
grid updates every 16 steps with a warm-up of 16, lr 1e-2, that file's three
lambdas, the model's default table; fit's schedule applied by hand as there.

"State" is every tensor of Trainer.state_dict() and the derived caches a step
reads: the f16 table mirror, the packed field fragments, the gate's.
"""
import math

import torch

from radnerf_amd import train_state as TS
from radnerf_amd.networks import MNGP, Ray_Gate
from radnerf_amd.sampler import cosine_lr
from radnerf_amd.trainer import Trainer

WH, N_IMG, R_SPHERE, HALF = (32, 32), 4, 0.25, 0.3
LAMBDAS = dict(lambda_cv_importance=1e-2, lambda_depth_mutual=1e-3, lambda_distortion=1e-3)
STEPS, EPOCHS, PER_EPOCH, LR, N_RAYS = 40, 2, 20, 1e-2, 512

_DATA = {}


def dataset(device):
    """directions (P, 3), poses (4, 3, 4), uint8 images (4, P, 3); built once"""
    key = str(device)
    if key in _DATA:
        return _DATA[key]
    W, H = WH
    y, x = torch.meshgrid(torch.linspace(-HALF, HALF, H), torch.linspace(-HALF, HALF, W),
                          indexing="ij")
    dirs = torch.stack([x.reshape(-1), y.reshape(-1), torch.ones(H * W)], -1)
    dirs = (dirs / dirs.norm(dim=1, keepdim=True)).contiguous()
    ang = torch.arange(N_IMG) * (2 * math.pi / N_IMG) + 0.3
    pos = 1.5 * torch.stack([torch.cos(ang), torch.sin(ang), 0.3 * torch.sin(3 * ang)], -1)
    fwd = -pos / pos.norm(dim=1, keepdim=True)
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd))
    right = right / right.norm(dim=1, keepdim=True)
    up = torch.linalg.cross(right, fwd)
    poses = torch.cat([torch.stack([right, up, fwd], 2), pos[:, :, None]], 2).contiguous()
    d = torch.einsum("pj,nij->npi", dirs, poses[:, :, :3])
    o = poses[:, None, :, 3].expand_as(d)
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - R_SPHERE ** 2)
    t = -b - torch.sqrt(disc.clamp_min(0))
    hit = (disc > 0) & (t > 0)
    nrm = o + t[..., None] * d
    nrm = nrm / nrm.norm(dim=-1, keepdim=True)
    img = torch.where(hit[..., None], 0.5 + 0.5 * nrm, torch.ones_like(nrm))
    u8 = (img * 255).round().to(torch.uint8).contiguous()
    _DATA[key] = (dirs.to(device), poses.to(device), u8.to(device))
    return _DATA[key]


def intrinsics():
    """the pinhole matrix of dataset()'s directions: x = (u - cx) / f over
    linspace(-HALF, HALF, W)"""
    W, H = WH
    f = (W - 1) / (2 * HALF)
    return torch.tensor([[f, 0.0, (W - 1) / 2], [0.0, f, (H - 1) / 2], [0.0, 0.0, 1.0]])


def trainer(device, K, scale, ext, model_seed=3, gate_seed=4, deterministic=True, **kw):
    dirs, poses, u8 = dataset(device)
    m = MNGP(scale, size=K, seed=model_seed).to(device)
    g = Ray_Gate(K, seed=gate_seed).to(device)
    args = dict(lr=LR, deterministic=deterministic, seed=3, update_interval=16, warmup_steps=16,
                images=u8, directions=dirs, poses=poses, optimize_ext=ext, **LAMBDAS)
    args.update(kw)
    return Trainer(m, g, N_RAYS, **args)


def other_trainer(device, K, scale, ext, **kw):
    """the trainer a state is loaded into: built on models with other seeds"""
    return trainer(device, K, scale, ext, model_seed=99, gate_seed=98, **kw)


def run_steps(tr, stop, losses=None):
    """step_sampled from tr.global_step up to `stop`, fit's schedule by hand;
    appends each step's loss terms (sorted by name) to `losses`"""
    while tr.global_step < stop:
        step = tr.global_step
        if step % PER_EPOCH == 0:
            tr.opt.param_groups[0]["lr"] = cosine_lr(LR, step // PER_EPOCH, EPOCHS)
        terms = tr.step_sampled()
        if losses is not None:
            losses.append(torch.stack([terms[k] for k in sorted(terms)]).clone())
    return losses


def full_state(tr):
    """{name: CPU tensor}: state_dict()'s tensors and the derived caches"""
    out = dict(TS.tensors({k: v for k, v in tr.state_dict().items() if k != "header"}))
    out["derived/params_f16"] = tr.model.xyz_encoder.params_f16().detach().cpu()
    out["derived/packed_frags"] = tr.model.packed_frags().detach().cpu()
    out["derived/gate_frags"] = tr.gate.packed_frags().detach().cpu()
    return out


def assert_same_tensors(a, b):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k in sorted(a):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def plain_part(state):
    """a state with its tensors replaced by their shapes: the plain values"""
    if torch.is_tensor(state):
        return ("tensor", tuple(state.shape), str(state.dtype))
    if isinstance(state, dict):
        return {k: plain_part(v) for k, v in state.items()}
    if isinstance(state, list):
        return [plain_part(v) for v in state]
    return state


def assert_same_state(a, b):
    """two state_dict()s: equal tensors (torch.equal), equal plain values,
    the header's sizes and checksums among them"""
    assert_same_tensors(dict(TS.tensors(a)), dict(TS.tensors(b)))
    assert plain_part(a) == plain_part(b)
