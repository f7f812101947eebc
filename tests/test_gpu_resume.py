"""GPU: a training run saved and resumed (Trainer.state_dict / load_state_dict /
save_state / load_state, fit_resumable(ckpt_dir=, resume=); radnerf_amd.train_state,
DESIGN.md §4 "Checkpoint and resume").

With Trainer(deterministic=True) a step is a function of the state and the
seed, bit for bit, so the bar is equality: a run cut at any step, its state
loaded into a trainer built on other models, continues with the loss terms and
ends in the state of the uninterrupted run -- every tensor of state_dict() and
the derived caches a step reads (the f16 table mirror, the packed fragments),
compared with torch.equal.  The set-up is tests/resume_ref.py's.

The cuts of test_resume_is_bit_exact: 7 inside the grid warm-up, 23 past it,
between two grid updates and in mid-epoch of 20 (the lr is the second
epoch's), 32 on a grid update.  The uninterrupted run of each shape is made
once and shared.
"""
import os

import pytest
import torch

import resume_ref as RR
from radnerf_amd import train_state as TS

pytestmark = pytest.mark.gpu

SHAPES = [(2, 0.5, False), (2, 0.5, True), (4, 16.0, True)]
CUTS = [7, 23, 32]
SEED = 1234

_WHOLE = {}


def _whole_run(cuda, K, scale, ext):
    """run A: 40 sampled steps, every step's loss terms, the final state"""
    key = (K, scale, ext)
    if key not in _WHOLE:
        torch.manual_seed(SEED)
        tr = RR.trainer(cuda, K, scale, ext)
        losses = RR.run_steps(tr, RR.STEPS, [])
        _WHOLE[key] = (torch.stack(losses).cpu(), RR.full_state(tr))
    return _WHOLE[key]


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("K,scale,ext", SHAPES)
def test_resume_is_bit_exact(cuda, K, scale, ext, cut):
    want_losses, want = _whole_run(cuda, K, scale, ext)
    torch.manual_seed(SEED)
    tr = RR.trainer(cuda, K, scale, ext)
    head = RR.run_steps(tr, cut, [])
    sd = tr.state_dict()
    del tr
    tr = RR.other_trainer(cuda, K, scale, ext)
    assert not torch.equal(tr.model.mlp_params.detach().cpu(), sd["model"]["mlp_params"])
    tr.load_state_dict(sd)
    assert tr.global_step == cut
    tail = RR.run_steps(tr, RR.STEPS, [])
    got_losses = torch.stack(head + tail).cpu()
    assert bool(torch.isfinite(want_losses).all())
    assert torch.equal(got_losses[:cut], want_losses[:cut])
    for step in range(cut, RR.STEPS):
        assert torch.equal(got_losses[step], want_losses[step]), step
    RR.assert_same_tensors(RR.full_state(tr), want)
    # the run moved after the cut: what is compared is not the loaded state
    assert not torch.equal(want["model/mlp_params"], sd["model"]["mlp_params"])
    if ext:
        assert float(want["poses/dR"].abs().max()) > 0


def test_resume_through_a_file(cuda, tmp_path):
    K, scale, ext, cut = 2, 0.5, True, 23
    want_losses, want = _whole_run(cuda, K, scale, ext)
    torch.manual_seed(SEED)
    tr = RR.trainer(cuda, K, scale, ext)
    RR.run_steps(tr, cut)
    sd = tr.state_dict()
    path = str(tmp_path / "state.pt")
    assert tr.save_state(path).wait() == path
    del tr
    tr = RR.other_trainer(cuda, K, scale, ext)
    tr.load_state(path)
    RR.assert_same_state(tr.state_dict(), sd)        # directly after loading
    tail = RR.run_steps(tr, RR.STEPS, [])
    assert torch.equal(torch.stack(tail).cpu(), want_losses[cut:])
    RR.assert_same_tensors(RR.full_state(tr), want)


def test_resume_with_cull_and_erode(cuda):
    K, scale, ext, cut = 2, 0.5, False, 23
    kw = dict(intrinsics=RR.intrinsics(), img_wh=RR.WH, cull_invisible=True, erode=True)
    torch.manual_seed(SEED)
    a = RR.trainer(cuda, K, scale, ext, **kw)
    assert a.model.count_grid is not None and int(a.n_culled.sum()) > 0
    want_losses = torch.stack(RR.run_steps(a, RR.STEPS, [])).cpu()
    want = RR.full_state(a)
    torch.manual_seed(SEED)
    b = RR.trainer(cuda, K, scale, ext, **kw)
    RR.run_steps(b, cut)
    sd = b.state_dict()
    assert "count_grid" in sd["model"]
    del b
    c = RR.other_trainer(cuda, K, scale, ext, **kw)
    c.model.count_grid.fill_(0.5)                     # what the file must replace
    c.load_state_dict(sd)
    tail = torch.stack(RR.run_steps(c, RR.STEPS, [])).cpu()
    assert torch.equal(tail, want_losses[cut:])
    got = RR.full_state(c)
    assert "model/count_grid" in got
    RR.assert_same_tensors(got, want)


def _pixel_run(cuda, stop, tr, picks, losses):
    dirs, poses, u8 = RR.dataset(cuda)
    while tr.global_step < stop:
        img, pix = picks[tr.global_step]
        target = u8[img.to(cuda), pix.to(cuda)].float() / 255
        terms = tr.step_pixels(img, pix, target)         # noise=None: torch's generator
        losses.append(torch.stack([terms[k] for k in sorted(terms)]).clone())
    return losses


def test_step_pixels_resume(cuda):
    """step_pixels with noise=None under random_bg: the march jitter and the
    background come from the device's generator, which the state carries."""
    K, scale, ext, steps, cut = 2, 16.0, True, 12, 5
    gen = torch.Generator().manual_seed(21)
    n_pix = RR.WH[0] * RR.WH[1]
    picks = [(torch.randint(RR.N_IMG, (RR.N_RAYS,), generator=gen),
              torch.randint(n_pix, (RR.N_RAYS,), generator=gen)) for _ in range(steps)]
    torch.manual_seed(SEED)
    a = RR.trainer(cuda, K, scale, ext, random_bg=True)
    want_losses = torch.stack(_pixel_run(cuda, steps, a, picks, [])).cpu()
    want = RR.full_state(a)
    torch.manual_seed(SEED)
    b = RR.trainer(cuda, K, scale, ext, random_bg=True)
    head = _pixel_run(cuda, cut, b, picks, [])
    sd = b.state_dict()
    del b
    torch.rand(7, device=cuda), torch.rand(5)            # the generators move on
    c = RR.other_trainer(cuda, K, scale, ext, random_bg=True)
    c.load_state_dict(sd)
    tail = _pixel_run(cuda, steps, c, picks, [])
    assert torch.equal(torch.stack(head + tail).cpu(), want_losses)
    RR.assert_same_tensors(RR.full_state(c), want)
    # the jitter did come from the generator: another seed, another run
    torch.manual_seed(SEED + 1)
    d = RR.trainer(cuda, K, scale, ext, random_bg=True)
    other = torch.stack(_pixel_run(cuda, 2, d, picks, [])).cpu()
    assert not torch.equal(other, want_losses[:2])


class _Stop(Exception):
    pass


def test_fit_resumes(cuda, tmp_path):
    K, scale, ext, epochs, per_epoch, keep = 2, 0.5, True, 3, 10, 2
    torch.manual_seed(SEED)
    a = RR.trainer(cuda, K, scale, ext)
    want_log = a.fit(epochs, per_epoch)
    want = RR.full_state(a)
    ckpt = str(tmp_path / "ckpt")

    def stop(entry):
        if entry["epoch"] == 1:
            raise _Stop

    torch.manual_seed(SEED)
    b = RR.trainer(cuda, K, scale, ext)
    with pytest.raises(_Stop):
        b.fit_resumable(epochs, per_epoch, ckpt_dir=ckpt, ckpt_every=1, keep=keep, callback=stop)
    assert b.global_step == 2 * per_epoch
    assert sorted(os.listdir(ckpt)) == [TS.checkpoint_name(1), TS.checkpoint_name(2)]
    del b
    c = RR.other_trainer(cuda, K, scale, ext)
    seen = []
    log = c.fit_resumable(epochs, per_epoch, ckpt_dir=ckpt, ckpt_every=1, keep=keep,
                          resume=True, callback=seen.append)
    assert [e["epoch"] for e in seen] == [2]            # only the last epoch ran
    assert c.global_step == epochs * per_epoch
    assert log == want_log and len(log) == epochs
    RR.assert_same_tensors(RR.full_state(c), want)
    assert sorted(os.listdir(ckpt)) == [TS.checkpoint_name(2), TS.checkpoint_name(3)]
    assert len(os.listdir(ckpt)) == keep
    # the last file is the finished run: resuming from it runs nothing more
    d = RR.other_trainer(cuda, K, scale, ext)
    assert d.fit_resumable(epochs, per_epoch, ckpt_dir=ckpt, resume=True) == want_log
    assert d.global_step == epochs * per_epoch
    with pytest.raises(ValueError, match="steps_per_epoch"):
        d.fit_resumable(epochs, per_epoch + 1, ckpt_dir=ckpt, resume=True)


def test_background_save_is_a_snapshot(cuda, tmp_path):
    K, scale, ext = 2, 0.5, True
    torch.manual_seed(SEED)
    a = RR.trainer(cuda, K, scale, ext)
    RR.run_steps(a, 15)
    want = RR.full_state(a)
    torch.manual_seed(SEED)
    b = RR.trainer(cuda, K, scale, ext)
    RR.run_steps(b, 10)
    sd = b.state_dict()
    path = str(tmp_path / "state.pt")
    handle = b.save_state(path, background=True)
    RR.run_steps(b, 15)                                  # runs at once, behind the snapshot
    assert handle.wait() == path
    RR.assert_same_state(TS.read_file(path), sd)
    RR.assert_same_tensors(RR.full_state(b), want)
    # a second save reuses the buffers; wait_saves joins it
    b.save_state(path, background=True)
    b.wait_saves()
    assert TS.read_file(path)["progress"]["global_step"] == 15
    assert [n for n in os.listdir(tmp_path)] == ["state.pt"]


def test_default_mode_resume(cuda):
    """deterministic=False: the state loads bit for bit; the next step differs
    from the uninterrupted trainer's only in the order of fp32 atomics."""
    K, scale, ext, cut = 2, 0.5, True, 23
    torch.manual_seed(SEED)
    a = RR.trainer(cuda, K, scale, ext, deterministic=False)
    assert not a.renderer.deterministic
    RR.run_steps(a, cut)
    sd = a.state_dict()
    b = RR.other_trainer(cuda, K, scale, ext, deterministic=False)
    b.load_state_dict(sd)
    RR.assert_same_state(b.state_dict(), sd)
    ta, tb = a.step_sampled(), b.step_sampled()
    assert sorted(ta) == sorted(tb)
    for k in sorted(ta):
        u, v = float(tb[k]), float(ta[k])
        print(f"{k}: resumed {u:.9g}, uninterrupted {v:.9g}")
        # tests/test_gpu_deterministic.py's bar for the fused loss
        assert abs(u - v) <= 1e-5 * max(1.0, abs(v)), (k, u, v)
