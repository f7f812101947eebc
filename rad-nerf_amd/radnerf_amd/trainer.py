"""The training step of train_ml.py (training_step :172-193 + the optimizer of
:138-153) on the fused renderer, data-parallel over torch.distributed: one
process per GPU, each rank renders its own ray batch (dist.shard_rays) with
full replicas; one flat-gradient all-reduce (RCCL over xGMI) per step, then
the fused Adam; the occupancy grids are updated every `update_interval`
steps with a rank-consistent random stream (dist.update_density_grid), so
parameters, density grids and bitfields stay bit-identical across ranks.

    tr = Trainer(model, gate, n_rays=8192, lr=1e-2, lambda_cv_importance=1e-2)
    for step in range(n):
        terms = tr.step(rays_o, rays_d, imgs_d, target_rgb)

With camera pose refinement (--optimize_ext, train_ml.py:90-93, 129-146) the
trainer owns the cameras and forms the rays itself from (image, pixel) picks;
the per-image corrections dR (axis-angle) / dT are parameters of the same
flat gradient buffer and the same Adam, in a group of their own:

    tr = Trainer(model, gate, n_rays=8192, directions=directions, poses=poses,
                 optimize_ext=True, pose_lr=1e-8)
    terms = tr.step_pixels(img_idxs, pix_idxs, target_rgb)

Validation (validation_step, train_ml.py:214-250) renders whole images of the
trainer's camera on the test-time chain and reports PSNR / SSIM
(radnerf_amd.evaluate, radnerf_amd.metrics); it leaves the training state alone:

    tr = Trainer(model, gate, n_rays=8192, directions=directions, poses=poses,
                 img_wh=(W, H))
    val = tr.validate(test_poses, test_images)      # {"psnr", "ssim", "per_image"}

With the training images on the device (uint8 or fp32, sampler.TrainImages)
the trainer also produces each step's inputs and runs the epoch loop
(datasets/base.py:23-31, train_ml.py:124-153,172-200,295-297):

    tr = Trainer(model, gate, n_rays=8192, directions=directions, poses=poses,
                 img_wh=(W, H), images=images_u8)        # (N, H*W, 3)
    terms = tr.step_sampled()         # one rn_sample_batch launch, then the step
    log = tr.fit(num_epochs=30, steps_per_epoch=1000, val_poses=test_poses,
                 val_images=test_images)

step_sampled draws the (image, pixel) picks, gathers the targets, forms the
rays (refined by dR / dT under optimize_ext) and fills the march jitter and
the random background in one launch, all from a counter-based hash of
(seed, global_step, rank): no torch generator, different pixels on every
rank, and a trainer resumed with the same seed and global_step continues the
same stream of batches.  (The batches repeat; the step's gradients repeat bit
for bit only with Trainer(deterministic=True), which replaces the step's fp32
sums in arrival order by ordered ones -- DESIGN.md §4 "Deterministic
training".)  The consumed batch stays in `tr.last_batch`.  step and
step_pixels keep drawing from torch's generator.  fit sets the cosine
schedule (sampler.cosine_lr, eta_min = lr / 30) on the network's parameter
group at each epoch's start (the pose group keeps its lr, as the reference
schedules only net_opt), accumulates the epoch's loss terms on the device,
reads them once per epoch for the log, and validates every `val_every` epochs
and after the last.

With the camera intrinsics the trainer culls the occupancy grids to the
training cameras' frusta once, before the first step (upstream ngp_pl's
mark_invisible_cells; MNGP.mark_invisible_cells), and the grid updates then
skip the culled cells; `erode` decays cells seen by few cameras faster
(networks.py:396-398):

    tr = Trainer(model, gate, n_rays=8192, directions=directions, poses=poses,
                 img_wh=(W, H), intrinsics=K, cull_invisible=True, erode=True)

The cull uses the initial poses.  Under optimize_ext it is not repeated: the
corrections move at lr 1e-8 and do not shift a frustum by a grid cell.

Out of scope: dataset file readers, the Lightning loop,
logging back-ends.
"""
import math

import torch

from . import dist as rdist
from .fused import FusedMLRenderer
from .optim import FusedAdam

MAX_SAMPLES = 1024


def _rank():
    """torch.distributed's rank when it is initialised, else 0"""
    import torch.distributed as td
    return td.get_rank() if td.is_available() and td.is_initialized() else 0


class Trainer:
    # fit(): where its validations write their images (validate's save_dir); None: nowhere
    val_save_dir = None

    def __init__(self, model, gating_net, n_rays, lr=1e-2, lambda_opacity=1e-3,
                 lambda_cv_importance=0.0, lambda_depth_mutual=0.0, exp_step_factor=None,
                 random_bg=False, update_interval=16, warmup_steps=256, seed=0,
                 bucketed=True, lambda_distortion=0.0, directions=None, poses=None,
                 optimize_ext=False, pose_lr=1e-8, img_wh=None, images=None, intrinsics=None,
                 cull_invisible=False, erode=False, deterministic=False):
        """deterministic=True: the renderer is FusedMLRenderer(deterministic=
        True) (ValueError above 8 sub-NeRFs).  With step_sampled / fit, whose
        batches are a hash of (seed, global_step, rank), every parameter, Adam
        moment, density grid, bitfield and loss term after any number of steps
        is then a function of the initial state and the seed, bit for bit, on
        one GPU in one process (step / step_pixels without `noise` still draw
        from torch's generator: seed it).  Under data parallelism each rank's
        local gradient is reproducible; the collective sums the ranks in
        RCCL's order, which this mode does not fix."""
        if optimize_ext and (directions is None or poses is None):
            raise ValueError("Trainer(optimize_ext=True) needs directions (P, 3) and poses "
                             "(N, 3, 4): the pose corrections are per image of `poses`")
        if (directions is None) != (poses is None):
            raise ValueError("Trainer: give directions and poses together")
        if img_wh is not None:
            if directions is None:
                raise ValueError("Trainer(img_wh=...) needs directions and poses: img_wh is the "
                                 "(W, H) of the camera `directions` describes")
            if len(img_wh) != 2 or int(img_wh[0]) * int(img_wh[1]) != directions.shape[0]:
                raise ValueError(f"Trainer: img_wh {tuple(img_wh)} does not match the "
                                 f"{directions.shape[0]} rows of directions")
        if cull_invisible and (intrinsics is None or poses is None or img_wh is None):
            raise ValueError("Trainer(cull_invisible=True) needs intrinsics (3x3), poses "
                             "(N, 3, 4) and img_wh (W, H): the cells are tested against "
                             "those cameras' frusta")
        if erode and not cull_invisible and getattr(model, "count_grid", None) is None:
            raise ValueError("Trainer(erode=True) needs cull_invisible=True (or a model "
                             "already marked by mark_invisible_cells): the erode decay "
                             "divides by the count_grid")
        if images is not None:
            from .sampler import TrainImages
            if directions is None:
                raise ValueError("Trainer(images=...) needs directions and poses: the images "
                                 "are those of `poses`, pixel by pixel of `directions`")
            if not isinstance(images, TrainImages):
                images = TrainImages(images)
            if images.n_images != poses.shape[0] or images.n_pix != directions.shape[0]:
                raise ValueError(f"Trainer: images are {images.n_images} x {images.n_pix} pixels "
                                 f"for {poses.shape[0]} poses and {directions.shape[0]} rows of "
                                 "directions")
        # step_sampled()'s training set and its reused batch buffers
        self.images, self.last_batch = images, None
        self.n_rays, self.lr0 = int(n_rays), float(lr)
        # validate()'s camera: (W, H) of `directions`
        self.img_wh = None if img_wh is None else (int(img_wh[0]), int(img_wh[1]))
        self._evaluator = None
        self.model, self.gate = model, gating_net
        self.device = model.mlp_params.device
        self.deterministic = bool(deterministic)
        self.renderer = FusedMLRenderer(model, gating_net, n_rays,
                                        deterministic=self.deterministic)
        # train_ml.py:101-102: exp step 1/256 beyond scale 0.5
        self.esf = (1 / 256 if model.scale > 0.5 else 0.0) if exp_step_factor is None \
            else float(exp_step_factor)
        self.random_bg = random_bg
        self.lambdas = dict(lambda_opacity=lambda_opacity,
                            lambda_cv_importance=lambda_cv_importance,
                            lambda_depth_mutual=lambda_depth_mutual,
                            lambda_distortion=lambda_distortion)
        params = [model.xyz_encoder.params, model.mlp_params, gating_net.params]
        # the cameras step_pixels forms rays from (train_ml.py:126-127)
        self.optimize_ext = bool(optimize_ext)
        self.directions = self.poses = self.mean_dir = None
        if directions is not None:
            if directions.ndim != 2 or directions.shape[1] != 3 or poses.ndim != 3 \
                    or tuple(poses.shape[1:]) != (3, 4):
                raise ValueError(f"Trainer: directions must be (P, 3) and poses (N, 3, 4), got "
                                 f"{tuple(directions.shape)} and {tuple(poses.shape)}")
            self.directions = directions.detach().to(self.device, torch.float32).contiguous()
            self.poses = poses.detach().to(self.device, torch.float32).contiguous()
        pose_params = []
        if self.optimize_ext:
            # train_ml.py:129-134: per-image axis-angle / translation corrections.
            # They follow the gate in the flat buffer, so [grid, MLP, gate] and
            # dist.step_ranges keep their offsets, and the ranks average the
            # pose gradients in the same collective.
            n_img = self.poses.shape[0]
            self.dR = torch.nn.Parameter(torch.zeros(n_img, 3, device=self.device))
            self.dT = torch.nn.Parameter(torch.zeros(n_img, 3, device=self.device))
            self.mean_dir = self.directions.mean(0).contiguous()
            pose_params = [self.dR, self.dT]
        # gradients live in one flat buffer: one collective per step
        self.grads = rdist.GradAllReduce(params + pose_params, self.device)
        for p, v in zip(params + pose_params, self.grads.views):
            p.grad = v
        groups = [dict(params=params)]
        if pose_params:
            # train_ml.py:146: FusedAdam([dR, dT], 1e-8) -- the hard-coded lr,
            # and apex's default eps (the network's 1e-15 is passed explicitly)
            groups.append(dict(params=pose_params, lr=pose_lr, eps=1e-8))
        self.opt = FusedAdam(groups, lr=lr, eps=1e-15)      # train_ml.py:143
        self.update_interval, self.warmup_steps, self.seed = update_interval, warmup_steps, seed
        # Adam as the epilogue of a bucketed all-reduce (dist.GradAllReduce.
        # reduce_and_step); False: one collective, a division, then Adam
        self.bucketed = bucketed
        self.global_step = 0
        # the grid updates' erode decay, and the one-off frustum cull (from the
        # initial poses: dR / dT at lr 1e-8 do not move a frustum by a cell)
        self.erode = bool(erode)
        self.n_culled = None
        if cull_invisible:
            self.n_culled = model.mark_invisible_cells(intrinsics, self.poses, self.img_wh)

    def _bg(self):
        """ml_rendering.py:192-198"""
        if self.esf == 0:
            return torch.ones(3, device=self.device)
        if self.random_bg:
            return torch.rand(3, device=self.device)
        return torch.zeros(3, device=self.device)

    def step(self, rays_o, rays_d, imgs_d, target_rgb, noise=None):
        """One training step on this rank's rays; returns {term: mean} (this rank)."""
        return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, None)

    def step_pixels(self, img_idxs, pix_idxs, target_rgb, noise=None):
        """One training step on this rank's (image, pixel) picks of the
        trainer's cameras (train_ml.py:84-96).  With optimize_ext the rays
        come from the refined poses (rays.pose_rays), the chain also
        differentiates the rays, and rn_get_rays_pose_bw writes the dR / dT
        gradients into their views of the flat buffer before the collective."""
        from . import rays as R
        if self.directions is None:
            raise ValueError("Trainer.step_pixels needs Trainer(directions=..., poses=...)")
        img_idxs = img_idxs.to(self.device, torch.int64).contiguous()
        pix_idxs = pix_idxs.to(self.device, torch.int64).contiguous()
        if not self.optimize_ext:
            rays_o, rays_d, imgs_d = R.batch_rays(self.directions, self.poses, img_idxs, pix_idxs)
            return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, None)
        with torch.no_grad():
            rays_o, rays_d, imgs_d = R.pose_rays(self.directions, self.poses, self.dR, self.dT,
                                                 img_idxs, pix_idxs, mean_dir=self.mean_dir)
        return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, (img_idxs, pix_idxs))

    def step_sampled(self, noise=None):
        """One training step on a batch the trainer draws itself from its
        device-resident images (Trainer(images=...)): sampler.sample_batch for
        the key (seed, global_step, rank) -- picks, targets, rays (refined
        under optimize_ext), march jitter, random background in one launch --
        then the step of step_pixels.  `noise` overrides the sampled jitter.
        The consumed batch is kept as self.last_batch (its buffers are reused
        by the next call)."""
        from .sampler import sample_batch
        if self.images is None:
            raise ValueError("Trainer.step_sampled needs Trainer(images=..., directions=..., "
                             "poses=...)")
        if self.mean_dir is None and self.gate.type == "image":
            self.mean_dir = self.directions.mean(0).contiguous()
        ext = self.optimize_ext
        b = self.last_batch = sample_batch(
            self.images, self.directions, self.poses, self.n_rays, self.model.size, self.seed,
            self.global_step, rank=_rank(),
            dR=self.dR.detach() if ext else None, dT=self.dT.detach() if ext else None,
            mean_dir=self.mean_dir if self.gate.type == "image" else None, out=self.last_batch)
        # ml_rendering.py:192-198: the random background only with exp stepping
        bg = b["bg"] if self.random_bg and self.esf != 0 else self._bg()
        return self._step(b["rays_o"], b["rays_d"], b["imgs_d"], b["target"],
                          b["noise"] if noise is None else noise,
                          (b["img_idxs"], b["pix_idxs"]) if ext else None, bg)

    def _step(self, rays_o, rays_d, imgs_d, target_rgb, noise, picks, bg=None):
        if self.global_step % self.update_interval == 0:
            rdist.update_density_grid(self.model, 0.01 * MAX_SAMPLES / 3 ** 0.5,
                                      self.global_step,
                                      warmup=self.global_step < self.warmup_steps,
                                      seed=self.seed, erode=self.erode)
        B, K = rays_o.shape[0], self.model.size
        if noise is None:
            noise = torch.rand(K, B, device=self.device)
        second = imgs_d if self.gate.type == "image" else rays_d
        if bg is None:
            bg = self._bg()
        self.grads.zero()
        v = self.grads.views
        if picks is None:
            terms, _ = self.renderer.train_step(rays_o, rays_d, second, target_rgb, noise,
                                                bg, exp_step_factor=self.esf,
                                                grid_grad=v[0], mlp_grad=v[1], gate_grad=v[2],
                                                **self.lambdas)
        else:
            from . import rays as R
            terms, _, (g_o, g_d, g_2) = self.renderer.train_step(
                rays_o, rays_d, second, target_rgb, noise, bg, exp_step_factor=self.esf,
                grid_grad=v[0], mlp_grad=v[1], gate_grad=v[2], input_grad=True, **self.lambdas)
            # the gate's second input is rays_d ("ray") or imgs_d ("image")
            if self.gate.type == "image":
                g_i = g_2.contiguous()
            else:
                g_d, g_i = g_d + g_2, None
            R.pose_rays_backward(self.directions, self.poses, self.dR.detach(), picks[0],
                                 picks[1], self.mean_dir, g_o, g_d, g_i, v[3], v[4])
        if self.bucketed:
            self.grads.reduce_and_step(self.opt)
        else:
            self.grads.reduce()
            self.opt.step()
        self.global_step += 1
        return terms

    def validate(self, poses, images, T_threshold=1e-4, save_dir=None, epoch=0, swap_rb=False,
                 hard_gate=False):
        """validation_step (train_ml.py:214-250) over (pose, image) pairs:
        poses (N, 3, 4) camera-to-world, used as they are (the test split's own
        poses: no dR / dT, as the reference), images (N, H*W, 3) fp32 (or a
        sequence of (H*W, 3)) of the trainer's camera.  Returns {"psnr": mean,
        "ssim": mean, "per_image": [{"psnr", "ssim"}, ...]}, device fp64
        scalars, with no host synchronisation.  Training state is untouched:
        no density-grid update, no step.  Each rank evaluates what it is
        given.
        save_dir: also write image i as `{i:03d}epoch{epoch}.png`, its
        gate-weighted depth as `..._d.png` (train_ml.py:238-248; swap_rb: red
        and blue exchanged, as the reference's files) and, with more than one
        sub-NeRF, the gate map as `..._g.png` (ImageEvaluator.images8,
        imageout.ImageSaver); the files are complete on return, the numbers
        are the same.  Without it nothing more is launched or allocated."""
        from .evaluate import ImageEvaluator
        from .metrics import ImageMetrics
        if self.directions is None or self.img_wh is None:
            raise ValueError("Trainer.validate needs Trainer(directions=..., poses=..., "
                             "img_wh=(W, H))")
        if min(self.img_wh) < 11:
            raise ValueError(f"Trainer.validate: img_wh {self.img_wh}: SSIM needs H and W of at "
                             "least 11 (one 11 x 11 window)")
        if not torch.is_tensor(poses) or poses.ndim != 3 or tuple(poses.shape[1:]) != (3, 4):
            raise ValueError(f"Trainer.validate: poses must be (N, 3, 4), got "
                             f"{tuple(getattr(poses, 'shape', ()))}")
        if len(images) != poses.shape[0]:
            raise ValueError(f"Trainer.validate: {len(images)} images for {poses.shape[0]} poses")
        n_pix = self.directions.shape[0]
        for i, im in enumerate(images):
            if not torch.is_tensor(im) or tuple(im.shape) != (n_pix, 3):
                raise ValueError(f"Trainer.validate: images[{i}] must be ({n_pix}, 3), got "
                                 f"{tuple(getattr(im, 'shape', ()))}")
            if im.dtype != torch.float32 or not im.is_contiguous():
                raise ValueError(f"Trainer.validate: images[{i}] must be contiguous float32")
        if self._evaluator is None:
            self._evaluator = ImageEvaluator(self.model, self.gate, self.directions, self.img_wh,
                                             exp_step_factor=self.esf)
        saver = None
        if save_dir is not None:
            from .imageout import ImageSaver
            saver = ImageSaver(save_dir)
        acc = ImageMetrics()
        for i, (pose, im) in enumerate(zip(poses, images)):
            im = im.to(self.device)
            rgb = self._evaluator.render_image(pose, T_threshold)["rgb"]
            acc.update(rgb, im, self.img_wh)
            if saver is not None:
                im8 = self._evaluator.images8(swap_rb=swap_rb, hard_gate=hard_gate)
                for kind, tail in (("rgb", ""), ("depth", "_d"), ("gate", "_g")):
                    if kind in im8:
                        saver.save(f"{i:03d}epoch{int(epoch)}{tail}.png", im8[kind], kind)
        if saver is not None:
            saver.flush()
        return acc.compute()

    def fit(self, num_epochs=30, steps_per_epoch=1000, val_poses=None, val_images=None,
            val_every=None, eta_min=None, callback=None):
        """The epoch loop of train_ml.py:124-153,172-200,295-297 on the
        trainer's device-resident images.  At the start of epoch e the
        network's parameter group gets sampler.cosine_lr(lr, e, num_epochs,
        eta_min) (eta_min None: lr / 30; the pose group keeps its lr); the
        epoch runs steps_per_epoch step_sampled() calls, summing the loss terms
        on the device, and reads them once at its end.  With val_poses /
        val_images (as validate takes them) the validation runs every
        val_every epochs (None: min(num_epochs, 10), as
        check_val_every_n_epoch) and after the last.  Returns one dict per
        epoch: epoch, lr, loss (the sum of the term means), terms {name: mean},
        train_psnr (-10 log10 of the epoch's mean rgb MSE, what the accumulated
        PeakSignalNoiseRatio(data_range=1) logs) and, where it ran, val
        {"psnr", "ssim"} as floats.  callback(entry) is called once per epoch.
        With `val_save_dir` set on the trainer (None by default) each
        validation also writes its images there, named by the epoch (validate's
        save_dir and epoch).
        The batches depend on (seed, global_step, rank) alone: a trainer
        resumed with the same seed and global_step continues the stream."""
        from .sampler import cosine_lr
        if self.images is None:
            raise ValueError("Trainer.fit needs Trainer(images=..., directions=..., poses=...)")
        num_epochs, steps = int(num_epochs), int(steps_per_epoch)
        if num_epochs < 1 or steps < 1:
            raise ValueError(f"Trainer.fit: num_epochs and steps_per_epoch must be at least 1, "
                             f"got {num_epochs} and {steps}")
        if (val_poses is None) != (val_images is None):
            raise ValueError("Trainer.fit: give val_poses and val_images together")
        if val_poses is not None and self.img_wh is None:
            raise ValueError("Trainer.fit(val_poses=...) needs Trainer(img_wh=(W, H))")
        val_every = min(num_epochs, 10) if val_every is None else int(val_every)
        if val_every < 1:
            raise ValueError(f"Trainer.fit: val_every must be at least 1, got {val_every}")
        if callback is not None and not callable(callback):
            raise ValueError("Trainer.fit: callback must be callable")
        log = []
        for epoch in range(num_epochs):
            lr = cosine_lr(self.lr0, epoch, num_epochs, eta_min)
            self.opt.param_groups[0]["lr"] = lr
            names, acc = None, None
            for _ in range(steps):
                terms = self.step_sampled()
                if names is None:
                    names = list(terms)
                    acc = torch.zeros(len(names), device=self.device, dtype=torch.float64)
                acc += torch.stack([terms[k] for k in names])
            means = (acc / steps).tolist()              # the epoch's one host read
            terms = dict(zip(names, means))
            entry = {"epoch": epoch, "lr": lr, "loss": sum(means), "terms": terms,
                     "train_psnr": -10.0 * math.log10(terms["rgb"]) if terms["rgb"] > 0
                     else math.inf}
            if val_poses is not None and ((epoch + 1) % val_every == 0
                                          or epoch == num_epochs - 1):
                val = self.validate(val_poses, val_images, save_dir=self.val_save_dir,
                                    epoch=epoch)
                entry["val"] = {k: float(val[k]) for k in ("psnr", "ssim")}
            log.append(entry)
            if callback is not None:
                callback(entry)
        return log
