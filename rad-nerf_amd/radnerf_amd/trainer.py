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
rank, and a trainer resumed by load_state / load_state_dict (which restore
global_step with everything else) continues the same stream of batches.  (The
batches repeat; the step's gradients repeat bit for bit only with
Trainer(deterministic=True), which replaces the step's fp32
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

The whole training state -- parameters, occupancy grids, pose corrections,
Adam moments and step counts, global_step, fit's epoch position and log,
torch's generator states -- is saved and restored by state_dict /
load_state_dict and, through a file, save_state / load_state
(radnerf_amd.train_state; Lightning's --ckpt_path and ModelCheckpoint).  With
deterministic=True the continued run equals the uninterrupted one bit for bit:

    tr.save_state("run/state.pt")                   # at any step
    h = tr.save_state("run/state.pt", background=True); ...; h.wait()
    tr2 = Trainer(...same arguments...); tr2.load_state("run/state.pt")
    log = tr.fit_resumable(30, 1000, ckpt_dir="run", ckpt_every=5)
    log = tr2.fit_resumable(30, 1000, ckpt_dir="run", resume=True)   # picks the run up

(fit keeps its argument list and is fit_resumable without checkpoints.)

export_reference / load_reference write and read the reference's slim
checkpoint (utils/util.py:33-43), with dR / dT under optimize_ext.

Out of scope: dataset file readers, the Lightning loop,
logging back-ends.
"""
import copy
import math
import numbers
import os

import torch

from . import dist as rdist
from . import train_state as TS
from .fused import FusedMLRenderer, route_params
from .optim import FusedAdam

MAX_SAMPLES = 1024


def _rank():
    """torch.distributed's rank when it is initialised, else 0"""
    import torch.distributed as td
    return td.get_rank() if td.is_available() and td.is_initialized() else 0


def _world():
    """torch.distributed's world size when it is initialised, else 1"""
    import torch.distributed as td
    return td.get_world_size() if td.is_available() and td.is_initialized() else 1


class Trainer:
    # fit(): where its validations write their images (validate's save_dir); None: nowhere
    val_save_dir = None
    # fit(): a radnerf_amd.lpips.LPIPS its validations also report (validate's lpips); None: off
    val_lpips = None
    # fit_resumable(ckpt_dir=...): write the checkpoints with save_state(background=True)
    ckpt_background = True
    # routed training (Trainer(gate_topk=, gate_min=, renormalize=,
    # route_from_step=)): the defaults keep every pair on every step
    gate_topk, gate_min, renormalize, route_from_step = None, 0.0, False, 0

    def __init__(self, model, gating_net, n_rays, lr=1e-2, lambda_opacity=1e-3,
                 lambda_cv_importance=0.0, lambda_depth_mutual=0.0, exp_step_factor=None,
                 random_bg=False, update_interval=16, warmup_steps=256, seed=0,
                 bucketed=True, lambda_distortion=0.0, directions=None, poses=None,
                 optimize_ext=False, pose_lr=1e-8, img_wh=None, images=None, intrinsics=None,
                 cull_invisible=False, erode=False, deterministic=False, gate_topk=None,
                 gate_min=0.0, renormalize=False, route_from_step=0, depths=None,
                 lambda_depth=0.0, lambda_depth_var=0.0, depth_clip=float("inf"), guided=False,
                 guided_tile=16, guided_uniform_frac=0.5, guided_alpha=0.5,
                 guided_refresh_every=16):
        """depths / lambda_depth / lambda_depth_var / depth_clip: depth
        supervision (DESIGN.md §4 "Depth supervision").  depths: the training
        set's depth maps (sampler.TrainDepths, or an (N, H*W) uint16 / fp32
        device tensor taken at scale 1, kind "t"), pixel by pixel of `images`;
        step_sampled / fit gather each batch's target ray parameters from its
        picks (rn_gather_depth), step and step_pixels take them from the caller
        (target_depth=).  lambda_depth weighs the squared error of the gated
        expected depth, lambda_depth_var the second moment of the
        ray-termination distribution about the target (each (t - z)^2 clipped
        at depth_clip^2); both are divided by the batch size, and a ray
        without a measurement (target <= 0) adds nothing.  ValueError for a
        negative lambda, depth_clip <= 0, or maps that do not match the
        images, before anything is allocated.
        gate_topk / gate_min / renormalize: routed training (FusedMLRenderer.
        forward; DESIGN.md §4 "Routed training") -- every step from global_step
        route_from_step on marches and differentiates only the (ray, sub-NeRF)
        pairs the gate keeps; the steps before it train dense, so the gate can
        form before it is cut.  `routing` hands the same three arguments to
        validate().  ValueError for gate_topk outside 1..K, gate_min outside
        [0, 1) or route_from_step < 0, before anything is allocated.
        deterministic=True: the renderer is FusedMLRenderer(deterministic=
        True) (ValueError above 8 sub-NeRFs).  With step_sampled / fit, whose
        batches are a hash of (seed, global_step, rank), every parameter, Adam
        moment, density grid, bitfield and loss term after any number of steps
        is then a function of the initial state and the seed, bit for bit, on
        one GPU in one process (step / step_pixels without `noise` still draw
        from torch's generator: seed it).  Under data parallelism each rank's
        local gradient is reproducible; the collective sums the ranks in
        RCCL's order, which this mode does not fix.
        guided=True: step_sampled / fit draw their batches through
        sampler.GuidedSampler (DESIGN.md §4 "Error-guided sampling") -- a
        share guided_uniform_frac of the rays uniformly, the rest in
        proportion to a guided_tile-pixel tiled map of the recent rgb error,
        every ray's seeds divided by its sampling density; the map moves by
        guided_alpha towards the recorded errors every guided_refresh_every
        steps.  Needs images and img_wh; ValueError for guided_uniform_frac
        outside (0, 1] (at 0 a pixel of a cell the map has written off would
        never be seen again), for the sampler's own limits, and under data
        parallelism (the ranks' maps would diverge).  step, step_pixels and
        validate are unchanged: their callers choose their own pixels."""
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
        from .fused import check_depth_weights
        check_depth_weights("Trainer", lambda_depth, lambda_depth_var, depth_clip)
        if depths is not None:
            from .sampler import TrainDepths
            if images is None:
                raise ValueError("Trainer(depths=...) needs images (and directions, poses): the "
                                 "maps are those of the training images, pixel by pixel")
            if not isinstance(depths, TrainDepths):
                depths = TrainDepths(depths)
            depths.check_images("Trainer", images)
        self.depths = depths
        self.depth_lambdas = dict(lambda_depth=float(lambda_depth),
                                  lambda_depth_var=float(lambda_depth_var),
                                  depth_clip=float(depth_clip))
        self._target_t = None       # step_sampled()'s reused target buffer
        self.guided = None
        self._guided_args = None
        if guided:
            from .sampler import guided_geometry
            fn = "Trainer(guided=True)"
            if images is None or img_wh is None:
                raise ValueError(f"{fn} needs images and img_wh (W, H): the error map is tiled "
                                 "over the training images")
            if not 0.0 < float(guided_uniform_frac) <= 1.0:
                raise ValueError(f"{fn}: guided_uniform_frac must be in (0, 1], got "
                                 f"{guided_uniform_frac!r}")
            if not 0.0 < float(guided_alpha) <= 1.0:
                raise ValueError(f"{fn}: guided_alpha must be in (0, 1], got {guided_alpha!r}")
            if isinstance(guided_refresh_every, bool) \
                    or not isinstance(guided_refresh_every, numbers.Integral) \
                    or guided_refresh_every < 1:
                raise ValueError(f"{fn}: guided_refresh_every must be an int >= 1, got "
                                 f"{guided_refresh_every!r}")
            guided_geometry(fn, images.n_images, images.n_pix, img_wh, guided_tile)
            if _world() > 1:
                raise ValueError(f"{fn} does not run under data parallelism (world size "
                                 f"{_world()}): each rank would build its own map")
            self._guided_args = dict(tile=int(guided_tile), uniform_frac=float(guided_uniform_frac),
                                     alpha=float(guided_alpha))
        self.guided_refresh_every = int(guided_refresh_every) if guided else 0
        # (one sub-NeRF: nothing to route, the arguments are accepted and ignored)
        route_params("Trainer", gating_net.out_dim, gate_topk, gate_min, renormalize)
        if isinstance(route_from_step, bool) or not isinstance(route_from_step, numbers.Integral) \
                or route_from_step < 0:
            raise ValueError(f"Trainer: route_from_step must be an int >= 0, got "
                             f"{route_from_step!r}")
        self.gate_topk = None if gate_topk is None else int(gate_topk)
        self.gate_min, self.renormalize = float(gate_min), bool(renormalize)
        self.route_from_step = int(route_from_step)
        # step_sampled()'s training set and its reused batch buffers
        self.images, self.last_batch = images, None
        self.n_rays, self.lr0 = int(n_rays), float(lr)
        # validate()'s camera: (W, H) of `directions`
        self.img_wh = None if img_wh is None else (int(img_wh[0]), int(img_wh[1]))
        # the 3x3 pinhole of `directions` (cull_invisible, export_mesh(method="tsdf"))
        self.intrinsics = intrinsics
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
        self.pose_lr = float(pose_lr)
        # fit's epoch position and log while it runs (state_dict's "progress");
        # the background save's buffers and writer (save_state)
        self._fit_progress = self._saver = None
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
        if self._guided_args is not None:
            from .sampler import GuidedSampler
            self.guided = GuidedSampler(images, self.img_wh, **self._guided_args)
        # steps recorded in the guided sampler's accumulators since its last refresh
        self._guided_pending = False

    @property
    def routing(self):
        """The routing this trainer trains with, as validate()'s and
        ImageEvaluator.render_image's keyword arguments: validate(poses,
        images, **trainer.routing) renders what was trained."""
        return {"gate_topk": self.gate_topk, "gate_min": self.gate_min,
                "renormalize": self.renormalize}

    def _route_now(self):
        """this step's routing arguments: dense before route_from_step"""
        return self.routing if self.global_step >= self.route_from_step else {}

    def _bg(self):
        """ml_rendering.py:192-198"""
        if self.esf == 0:
            return torch.ones(3, device=self.device)
        if self.random_bg:
            return torch.rand(3, device=self.device)
        return torch.zeros(3, device=self.device)

    def _depth_on(self):
        # (a trainer assembled before the option existed has no attribute)
        d = getattr(self, "depth_lambdas", None)
        return d is not None and (d["lambda_depth"] > 0 or d["lambda_depth_var"] > 0)

    def _depth_args(self, fn, n_rays, target_depth):
        """train_step's depth arguments for this step: none with both lambdas
        0 (the targets are then not looked at); ValueError for a lambda > 0
        without targets or targets that are not (n_rays,) fp32"""
        if not self._depth_on():
            return {}
        from .fused import check_depth_args
        check_depth_args(fn, n_rays, target_depth, **self.depth_lambdas,
                         device=getattr(self, "device", None))
        return dict(target_depth=target_depth, **self.depth_lambdas)

    def step(self, rays_o, rays_d, imgs_d, target_rgb, noise=None, target_depth=None):
        """One training step on this rank's rays; returns {term: mean} (this rank).
        target_depth ((B,) fp32 ray parameters, <= 0: no measurement): the
        depth terms' targets (Trainer(lambda_depth=, lambda_depth_var=))."""
        depth = self._depth_args("Trainer.step", rays_o.shape[0], target_depth)
        return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, None, depth=depth)

    def step_pixels(self, img_idxs, pix_idxs, target_rgb, noise=None, target_depth=None):
        """One training step on this rank's (image, pixel) picks of the
        trainer's cameras (train_ml.py:84-96).  With optimize_ext the rays
        come from the refined poses (rays.pose_rays), the chain also
        differentiates the rays, and rn_get_rays_pose_bw writes the dR / dT
        gradients into their views of the flat buffer before the collective."""
        from . import rays as R
        if self.directions is None:
            raise ValueError("Trainer.step_pixels needs Trainer(directions=..., poses=...)")
        depth = self._depth_args("Trainer.step_pixels", img_idxs.shape[0], target_depth)
        img_idxs = img_idxs.to(self.device, torch.int64).contiguous()
        pix_idxs = pix_idxs.to(self.device, torch.int64).contiguous()
        if not self.optimize_ext:
            rays_o, rays_d, imgs_d = R.batch_rays(self.directions, self.poses, img_idxs, pix_idxs)
            return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, None, depth=depth)
        with torch.no_grad():
            rays_o, rays_d, imgs_d = R.pose_rays(self.directions, self.poses, self.dR, self.dT,
                                                 img_idxs, pix_idxs, mean_dir=self.mean_dir)
        return self._step(rays_o, rays_d, imgs_d, target_rgb, noise, (img_idxs, pix_idxs),
                          depth=depth)

    def step_sampled(self, noise=None):
        """One training step on a batch the trainer draws itself from its
        device-resident images (Trainer(images=...)): sampler.sample_batch for
        the key (seed, global_step, rank) -- picks, targets, rays (refined
        under optimize_ext), march jitter, random background in one launch --
        then the step of step_pixels.  `noise` overrides the sampled jitter.
        The consumed batch is kept as self.last_batch (its buffers are reused
        by the next call).  The key is all the stream depends on: a trainer
        restored by load_state / load_state_dict has the saved global_step and
        draws the batches the saved run would have drawn next."""
        from .sampler import sample_batch
        if self.images is None:
            raise ValueError("Trainer.step_sampled needs Trainer(images=..., directions=..., "
                             "poses=...)")
        if self._depth_on() and self.depths is None:
            raise ValueError("Trainer.step_sampled: lambda_depth / lambda_depth_var > 0 need "
                             "Trainer(depths=...)")
        if self.mean_dir is None and self.gate.type == "image":
            self.mean_dir = self.directions.mean(0).contiguous()
        ext = self.optimize_ext
        gs = getattr(self, "guided", None)
        if gs is None:
            draw, head = sample_batch, (self.images,)
        else:
            # the map follows the errors recorded since its last refresh,
            # before this step's batch is drawn from it
            if self.global_step % self.guided_refresh_every == 0 and self._guided_pending:
                gs.refresh()
                self._guided_pending = False
            draw, head = gs.sample, ()
        b = self.last_batch = draw(
            *head, self.directions, self.poses, self.n_rays, self.model.size, self.seed,
            self.global_step, rank=_rank(),
            dR=self.dR.detach() if ext else None, dT=self.dT.detach() if ext else None,
            mean_dir=self.mean_dir if self.gate.type == "image" else None, out=self.last_batch)
        # ml_rendering.py:192-198: the random background only with exp stepping
        bg = b["bg"] if self.random_bg and self.esf != 0 else self._bg()
        weights = {} if gs is None else dict(ray_weight=b["ray_weight"],
                                             guided=(gs, b["cell_idx"]))
        depth = {}
        if self._depth_on():
            # the targets of this batch's picks, whichever sampler drew them
            from .sampler import gather_depth
            self._target_t = gather_depth(self.depths, self.directions, b["img_idxs"],
                                          b["pix_idxs"], out=self._target_t)
            depth = dict(target_depth=self._target_t, **self.depth_lambdas)
        terms = self._step(b["rays_o"], b["rays_d"], b["imgs_d"], b["target"],
                           b["noise"] if noise is None else noise,
                           (b["img_idxs"], b["pix_idxs"]) if ext else None, bg, weights, depth)
        if gs is not None:
            self._guided_pending = True
        return terms

    def _step(self, rays_o, rays_d, imgs_d, target_rgb, noise, picks, bg=None, weights=None,
              depth=None):
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
                                                **self.lambdas, **self._route_now(),
                                                **(weights or {}), **(depth or {}))
        else:
            from . import rays as R
            terms, _, (g_o, g_d, g_2) = self.renderer.train_step(
                rays_o, rays_d, second, target_rgb, noise, bg, exp_step_factor=self.esf,
                grid_grad=v[0], mlp_grad=v[1], gate_grad=v[2], input_grad=True, **self.lambdas,
                **self._route_now(), **(weights or {}), **(depth or {}))
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

    # ------------------------------------------------------- the training state
    def _named_params(self):
        """the optimiser's parameters under the names the state files them by"""
        out = [("xyz_encoder.params", self.model.xyz_encoder.params),
               ("mlp_params", self.model.mlp_params), ("gating_net.params", self.gate.params)]
        if self.optimize_ext:
            out += [("dR", self.dR), ("dT", self.dT)]
        return out

    def _structure(self):
        """What a state must match exactly.  The world size counts: the batch
        stream is a function of the rank."""
        m = self.model
        return {"K": int(m.size), "scale": float(m.scale), "cascades": int(m.cascades),
                "grid_size": int(m.grid_size), "table_len": int(m.xyz_encoder.params.numel()),
                "gate_out_dim": int(self.gate.out_dim), "gate_type": str(self.gate.type),
                "optimize_ext": bool(self.optimize_ext),
                "n_images": 0 if self.poses is None else int(self.poses.shape[0]),
                "world_size": _world()}

    def _dense_hyper(self):
        """the routing fields of a trainer that keeps every pair"""
        return {"gate_topk": int(self.gate.out_dim), "gate_min": 0.0, "renormalize": False,
                "route_from_step": 0}

    @staticmethod
    def _no_depth_hyper():
        """the depth fields of a trainer without depth supervision"""
        return {"lambda_depth": 0.0, "lambda_depth_var": 0.0, "depth_clip": float("inf")}

    def _route_hyper(self):
        """this trainer's (gate_topk None is all of them)"""
        k = self.gate.out_dim if self.gate_topk is None else self.gate_topk
        return {"gate_topk": int(k), "gate_min": float(self.gate_min),
                "renormalize": bool(self.renormalize),
                "route_from_step": int(self.route_from_step)}

    def _hyper(self):
        """What a state must match unless load_state(override=True)."""
        h = {"n_rays": int(self.n_rays), "seed": int(self.seed),
             "update_interval": int(self.update_interval),
             "warmup_steps": int(self.warmup_steps), "lr0": float(self.lr0),
             "pose_lr": float(self.pose_lr), "esf": float(self.esf),
             "random_bg": bool(self.random_bg), "erode": bool(self.erode),
             "deterministic": bool(self.deterministic)}
        h.update({k: float(v) for k, v in self.lambdas.items()})
        # the routing joins the table when it is set: a dense trainer's state
        # keeps the fields it had before routing existed, and a state without
        # them loads as dense (_load fills them in)
        route = self._route_hyper()
        if route != self._dense_hyper():
            h.update(route)
        # and so do the depth terms' weights and clip
        if self._depth_on():
            h.update(self.depth_lambdas)
        # likewise the guided sampler's: absent from an unguided trainer's state
        gs = getattr(self, "guided", None)
        if gs is not None:
            h.update({"guided": True, "guided_tile": int(gs.tile),
                      "guided_uniform_frac": float(gs.uniform_frac),
                      "guided_alpha": float(gs.alpha),
                      "guided_refresh_every": int(self.guided_refresh_every)})
        for i, g in enumerate(self.opt.param_groups):
            h[f"adam.{i}.betas"] = [float(b) for b in g["betas"]]
            h[f"adam.{i}.eps"] = float(g["eps"])
        return h

    def _build_state(self, fetch):
        """The state without its header.  fetch(name, device tensor) -> the
        host tensor that holds (state_dict) or will hold (a background save)
        its values; everything else is read here, at the call."""
        m = self.model
        model = {name: fetch("model/" + name, p) for name, p in self._named_params()[:3]}
        names = ["center", "xyz_min", "xyz_max", "half_size"]
        for i in range(m.size):
            names += [f"density_grid_{i}", f"density_bitfield_{i}"]
        if getattr(m, "count_grid", None) is not None:
            names.append("count_grid")
        for name in names:
            model[name] = fetch("model/" + name, getattr(m, name))
        state = {"structure": self._structure(), "hyper": self._hyper(), "model": model}
        if self.optimize_ext:
            state["poses"] = {"dR": fetch("poses/dR", self.dR), "dT": fetch("poses/dT", self.dT)}
        gs = getattr(self, "guided", None)
        if gs is not None:
            # the map and what was recorded since its last refresh; w and cdf
            # are recomputed on load
            state["guided"] = {k: fetch("guided/" + k, getattr(gs, k))
                               for k in ("emap", "acc_sum", "acc_cnt")}
        per_param = {}
        for name, p in self._named_params():
            st = self.opt.state.get(p) or {}
            per_param[name] = {"step": int(st.get("step", 0))}
            for mom in ("exp_avg", "exp_avg_sq"):
                t = st[mom] if mom in st else torch.zeros_like(p)
                per_param[name][mom] = fetch(f"optimizer/{name}/{mom}", t)
        state["optimizer"] = {"state": per_param,
                              "groups": [{"lr": float(g["lr"])} for g in self.opt.param_groups]}
        state["progress"] = {"global_step": int(self.global_step)}
        fit = getattr(self, "_fit_progress", None)
        if fit is not None:
            state["progress"]["fit"] = copy.deepcopy(fit)
        # step / step_pixels without `noise`, and _bg() under random_bg, draw from these
        state["generators"] = {"cpu": torch.get_rng_state().clone()}
        if self.device.type == "cuda":
            state["generators"]["device"] = torch.cuda.get_rng_state(self.device).clone()
        return state

    def state_dict(self):
        """The whole training state (radnerf_amd.train_state): a nested dict
        of CPU tensors and plain int / float / str / bool / list / dict values
        and nothing else, sealed with a header of per-tensor sizes and
        checksums.  The renderer's workspaces and plans, the fixed-point
        scales, the f16 table mirror, the packed fragments, the evaluator and
        last_batch are not part of it: they are rebuilt."""
        return TS.seal(self._build_state(lambda name, t: t.detach().to("cpu", copy=True)))

    def load_state_dict(self, state, override=False):
        """Restore the trainer from a state_dict().  Checked before anything is
        touched: the header and every tensor's checksum; the structure (K,
        scale, cascades, grid and table sizes, gate, optimize_ext and the
        number of images, world size), which must match; the hyper-parameters,
        which must match unless `override` (this trainer's then stand).  Each
        failure is a ValueError listing what differs with both values.
        Parameters are written in place, so the f16 mirror and the fragments
        are remade from the loaded fp32 values."""
        self._load(state, override, "the state", verified=False)

    def _load(self, state, override, where, verified):
        self.wait_saves()
        if not verified:
            TS.verify(state, where)
        # a state without the routing fields was trained dense, one without
        # the depth fields without depth supervision
        dense = {**self._dense_hyper(), **self._no_depth_hyper()}
        TS.check_compatible({**state, "hyper": {**dense, **state.get("hyper", {})}},
                            self._structure(), {**dense, **self._hyper()}, override, where)
        m, dev = self.model, self.device
        copies, moments = [], []

        def match(dst, src, name):
            if not torch.is_tensor(src) or src.numel() != dst.numel() or src.dtype != dst.dtype:
                raise ValueError(f"{where}: {name} is {tuple(getattr(src, 'shape', ()))} "
                                 f"{getattr(src, 'dtype', None)}, this trainer's is "
                                 f"{tuple(dst.shape)} {dst.dtype}")
            return src.reshape(dst.shape)

        try:
            saved = state["model"]
            names = ["center", "xyz_min", "xyz_max", "half_size"]
            for i in range(m.size):
                names += [f"density_grid_{i}", f"density_bitfield_{i}"]
            for name, p in self._named_params()[:3]:
                copies.append((p, match(p, saved[name], name)))
            for name in names:
                copies.append((getattr(m, name), match(getattr(m, name), saved[name], name)))
            if self.optimize_ext:
                for name in ("dR", "dT"):
                    p = getattr(self, name)
                    copies.append((p, match(p, state["poses"][name], name)))
            per_param = state["optimizer"]["state"]
            for name, p in self._named_params():
                st = per_param[name]
                moments.append((p, int(st["step"]), match(p, st["exp_avg"], name + ".exp_avg"),
                                match(p, st["exp_avg_sq"], name + ".exp_avg_sq")))
            lrs = [float(g["lr"]) for g in state["optimizer"]["groups"]]
            if len(lrs) != len(self.opt.param_groups):
                raise ValueError(f"{where}: {len(lrs)} optimiser groups, this trainer has "
                                 f"{len(self.opt.param_groups)}")
            count = saved.get("count_grid")
            if count is not None and tuple(count.shape) != (m.cascades, m.grid_size ** 3):
                raise ValueError(f"{where}: count_grid is {tuple(count.shape)}")
            global_step = int(state["progress"]["global_step"])
            gens = state["generators"]
            gs = getattr(self, "guided", None)
            # (a state of the other kind got here under override=True: this
            # trainer's sampling stands, a guided one starts a fresh map)
            gmap = state.get("guided") if gs is not None else None
            if gmap is not None:
                gmap = {k: match(getattr(gs, k), gmap[k], "guided/" + k)
                        for k in ("emap", "acc_sum", "acc_cnt")}
        except KeyError as e:
            raise ValueError(f"{where}: the state has no {e.args[0]!r}") from e
        # everything checked: write
        with torch.no_grad():
            for dst, src in copies:
                dst.copy_(src.to(dev))              # in place: _param_key changes
        m._set_box_host()
        m.count_grid = None if count is None else count.to(dev, copy=True)
        for p, step, avg, sq in moments:
            self.opt.state[p] = {"step": step, "exp_avg": avg.to(dev, copy=True),
                                 "exp_avg_sq": sq.to(dev, copy=True)}
        for g, lr in zip(self.opt.param_groups, lrs):
            g["lr"] = lr
        if gs is not None:
            if gmap is None:
                gs.reset()
            else:
                gs.load_state_dict(gmap)
            # a refresh of empty accumulators changes nothing, so the first
            # step at a refresh boundary may always run one
            self._guided_pending = True
        self.global_step = global_step
        self._fit_progress = copy.deepcopy(state["progress"].get("fit"))
        torch.set_rng_state(gens["cpu"])
        if dev.type == "cuda" and "device" in gens:
            torch.cuda.set_rng_state(gens["device"], dev)
        # rebuilt as at a fresh start: the batch buffers, the evaluator, and the
        # fixed-point scales (zeros: the first step measures the records in fp32)
        self.last_batch = self._evaluator = None
        ws = getattr(getattr(self, "renderer", None), "ws", None)
        if ws is not None:
            ws._fx, ws.fx_i = None, 0

    def save_state(self, path, background=False, _after=None):
        """state_dict() into a file (torch.save; written under a temporary
        name of the same directory, then os.replace).  Returns a handle whose
        wait() gives the path once the file is in place.
        background=True: the call copies the device state into a staging copy
        on the training stream, queues its copy to reused pinned host buffers
        on a side stream, hands checksums and writing to a writer thread, and
        returns; the next step may run at once, and the file holds the state
        at the call whatever ran after it.  A second save waits for the
        first; wait_saves(), load_state and interpreter exit wait for a
        pending write."""
        self.wait_saves()
        if not background:
            handle = TS.SaveHandle(TS.write_file(self.state_dict(), path))
            if _after is not None:
                _after()
            return handle
        if getattr(self, "_saver", None) is None:
            self._saver = TS.BackgroundSaver(self.device)
        return self._saver.save(self._build_state, path, after=_after)

    def wait_saves(self):
        """Join the writer of a background save; raises what it raised."""
        if getattr(self, "_saver", None) is not None:
            self._saver.wait()

    def load_state(self, path, override=False):
        """load_state_dict from a save_state file, read with torch.load(...,
        weights_only=True): nothing of the file is executed.  A wrong format
        version, a truncated file or a tensor failing its checksum raises
        ValueError naming the file (and the tensor)."""
        self.wait_saves()
        self._load(TS.read_file(path), override, str(path), verified=True)

    def export_reference(self, path, save_poses=None):
        """The reference's slim checkpoint (utils/util.py:33-43 of the
        Lightning state_dict): checkpoint.reference_state_dict's keys without
        model.grid_coords, flat, plus dR / dT under optimize_ext and, with
        save_poses (None: optimize_ext, as train_ml.py calls slim_ckpt), the
        training poses."""
        from .checkpoint import reference_state_dict
        ext = self.optimize_ext
        save_poses = ext if save_poses is None else bool(save_poses)
        if save_poses and self.poses is None:
            raise ValueError("Trainer.export_reference(save_poses=True) needs Trainer(poses=...)")
        sd = reference_state_dict(self.model, self.gate, slim=True,
                                  dR=self.dR if ext else None, dT=self.dT if ext else None,
                                  poses=self.poses if save_poses else None)
        return TS.atomic_save(sd, path)

    def load_reference(self, path):
        """The inverse of export_reference (checkpoint.load_reference_state;
        also a full Lightning checkpoint).  Where the file holds dR / dT they
        are loaded too; the optimiser's state is left alone."""
        from .checkpoint import load_reference_state
        state = torch.load(path, map_location="cpu", weights_only=True)
        sd = state["state_dict"] if "state_dict" in state else state
        poses = {k: sd[k] for k in ("dR", "dT") if k in sd}
        if poses:
            if not self.optimize_ext or set(poses) != {"dR", "dT"}:
                raise ValueError(f"{path}: holds the pose corrections {sorted(poses)}; this "
                                 f"trainer has optimize_ext={self.optimize_ext}")
            for k, v in poses.items():
                if tuple(v.shape) != tuple(getattr(self, k).shape):
                    raise ValueError(f"{path}: {k} is {tuple(v.shape)}, this trainer's is "
                                     f"{tuple(getattr(self, k).shape)}")
        load_reference_state(self.model, self.gate, state=state)
        with torch.no_grad():
            for k, v in poses.items():
                getattr(self, k).copy_(v.to(self.device, torch.float32))

    def export_mesh(self, path, method="density", poses=None, **kw):
        """The model's surface as a .ply / .obj file; returns the Mesh.  Reads
        the model only: parameters, grids and the optimiser's state are left as
        they are.
        method="density" (the default): the iso-surface of the density lattice
        (mesh.extract_mesh's arguments: resolution, iso, aabb, weights, normals,
        colors, and for the clean-up occupancy, keep_largest, min_vertices,
        min_fraction).
        method="tsdf": what the model renders, fused from depth images
        (tsdf.fuse_mesh's arguments) of this trainer's camera -- directions,
        img_wh, intrinsics -- from `poses` ((N, 3, 4); None: the training
        poses, as given, without dR / dT), rendered with this trainer's
        `routing` and exp_step_factor unless kw overrides them.  ValueError
        naming what is missing when the trainer was built without directions /
        poses, img_wh or intrinsics."""
        if method == "density":
            if poses is not None:
                raise ValueError("Trainer.export_mesh: poses belong to method=\"tsdf\"; the "
                                 "density method renders nothing")
            from .mesh import extract_mesh
            mesh = extract_mesh(self.model, **kw)
        elif method == "tsdf":
            missing = [name for name, v in (("directions", self.directions),
                                            ("img_wh", self.img_wh),
                                            ("intrinsics", self.intrinsics)) if v is None]
            if poses is None and self.poses is None:
                missing.append("poses")
            if missing:
                raise ValueError("Trainer.export_mesh(method=\"tsdf\") needs Trainer("
                                 + ", ".join(f"{m}=..." for m in missing) + "): the depth "
                                 "images are rendered from those cameras")
            from .tsdf import fuse_mesh
            args = dict(self.routing, exp_step_factor=self.esf)
            args.update(kw)
            mesh = fuse_mesh(self.model, self.gate, self.poses if poses is None else poses,
                             self.directions, self.img_wh, self.intrinsics, **args)
        else:
            raise ValueError(f"Trainer.export_mesh: method must be \"density\" or \"tsdf\", got "
                             f"{method!r}")
        mesh.save(path)
        return mesh

    def validate(self, poses, images, T_threshold=1e-4, save_dir=None, epoch=0, swap_rb=False,
                 hard_gate=False, gate_min=0.0, gate_topk=None, renormalize=False, lpips=None):
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
        are the same.  Without it nothing more is launched or allocated.
        gate_min / gate_topk / renormalize: the gate-sparse render of
        ImageEvaluator.render_image (sparse_gate.py); the defaults render every
        sub-NeRF on every ray.
        lpips: a radnerf_amd.lpips.LPIPS of the camera's size (--eval_lpips):
        "lpips" joins the mean and every per_image entry; None (the default)
        launches and allocates nothing more and returns exactly the keys
        above."""
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
        if lpips is not None:
            from .lpips import check_metric
            check_metric("Trainer.validate", lpips, self.img_wh)
        if self._evaluator is None:
            self._evaluator = ImageEvaluator(self.model, self.gate, self.directions, self.img_wh,
                                             exp_step_factor=self.esf)
        saver = None
        if save_dir is not None:
            from .imageout import ImageSaver
            saver = ImageSaver(save_dir)
        acc = ImageMetrics(lpips=lpips)
        for i, (pose, im) in enumerate(zip(poses, images)):
            im = im.to(self.device)
            rgb = self._evaluator.render_image(pose, T_threshold, gate_min=gate_min,
                                               gate_topk=gate_topk,
                                               renormalize=renormalize)["rgb"]
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
        """fit_resumable without checkpoints: the epoch loop from epoch 0 to
        the end, nothing written, nothing loaded (the arguments and the
        returned log are fit_resumable's)."""
        return self.fit_resumable(num_epochs, steps_per_epoch, val_poses, val_images, val_every,
                                  eta_min, callback)

    def fit_resumable(self, num_epochs=30, steps_per_epoch=1000, val_poses=None, val_images=None,
                      val_every=None, eta_min=None, callback=None, ckpt_dir=None,
                      ckpt_every=None, keep=2, resume=False):
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
        save_dir and epoch); with `val_lpips` set (a radnerf_amd.lpips.LPIPS,
        None by default) each validation entry also holds "lpips".
        The batches depend on (seed, global_step, rank) alone, so a run
        resumed by fit_resumable(..., resume=...) (load_state underneath)
        continues the stream.
        ckpt_dir: rank 0 writes the whole training state there as
        state_epochNNNN.pt (NNNN finished epochs) after every `ckpt_every`
        epochs (None: val_every) and after the last, once the epoch's log
        entry is complete and before the callback; in the background
        (save_state(background=True)) unless `ckpt_background` is False on the
        trainer.  Only the newest `keep` files stay.  The last write is waited
        for before the call returns.
        resume=True: load the newest complete file of ckpt_dir (none: start
        fresh); resume=path: load that file.  The run continues at the saved
        next epoch on the same schedule and returns the whole log, saved
        entries included.  A num_epochs, steps_per_epoch or eta_min other than
        the saved ones raises ValueError before anything is loaded or
        rendered.  Under data parallelism every rank loads the same file and
        no rank waits for another to save."""
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
        if ckpt_every is not None and ckpt_dir is None:
            raise ValueError("Trainer.fit_resumable: ckpt_every needs ckpt_dir, the directory the "
                             "checkpoints are written to")
        ckpt_every = val_every if ckpt_every is None else int(ckpt_every)
        if ckpt_every < 1:
            raise ValueError(f"Trainer.fit_resumable: ckpt_every must be at least 1, got "
                             f"{ckpt_every}")
        keep = int(keep)
        if keep < 1:
            raise ValueError(f"Trainer.fit_resumable: keep must be at least 1, got {keep}")
        if resume is True and ckpt_dir is None:
            raise ValueError("Trainer.fit_resumable(resume=True) needs ckpt_dir, the directory "
                             "whose newest file is loaded (or resume=path)")
        # as it is filed and compared: eta_min None is lr / 30 (sampler.cosine_lr)
        mine = {"num_epochs": num_epochs, "steps_per_epoch": steps,
                "eta_min": self.lr0 / 30 if eta_min is None else float(eta_min)}
        log, first = [], 0
        if resume:
            found = TS.newest_checkpoint(ckpt_dir) if resume is True \
                else (str(resume), TS.read_file(resume))
            if found is not None:
                path, state = found
                saved = state.get("progress", {}).get("fit")
                if saved is None:
                    raise ValueError(f"{path}: holds no epoch position (it was not written by "
                                     "fit_resumable); load it with load_state")
                diff = TS.differences({k: saved.get(k) for k in mine}, mine)
                if diff:
                    raise ValueError(f"{path}: the call has another schedule -- "
                                     + "; ".join(f"{k}: saved {u!r}, this call {v!r}"
                                                 for k, u, v in diff))
                self._load(state, False, path, verified=True)
                first, log = int(saved["next_epoch"]), copy.deepcopy(saved["log"])
        try:
            self._fit_epochs(first, log, mine, steps, eta_min, val_poses, val_images, val_every,
                             callback, ckpt_dir, ckpt_every, keep)
        finally:
            self._fit_progress = None       # absent outside fit
            self.wait_saves()
        return log

    def _fit_epochs(self, first, log, mine, steps, eta_min, val_poses, val_images, val_every,
                    callback, ckpt_dir, ckpt_every, keep):
        from .sampler import cosine_lr
        num_epochs = mine["num_epochs"]
        for epoch in range(first, num_epochs):
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
                # (lpips only when it is set: off, the call is the one without it)
                more = {} if self.val_lpips is None else {"lpips": self.val_lpips}
                val = self.validate(val_poses, val_images, save_dir=self.val_save_dir,
                                    epoch=epoch, **more)
                entry["val"] = {k: float(val[k]) for k in ("psnr", "ssim", *more)}
            log.append(entry)
            self._fit_progress = dict(mine, next_epoch=epoch + 1, log=log)
            if ckpt_dir is not None and _rank() == 0 and (
                    (epoch + 1) % ckpt_every == 0 or epoch == num_epochs - 1):
                os.makedirs(ckpt_dir, exist_ok=True)
                self.save_state(os.path.join(ckpt_dir, TS.checkpoint_name(epoch + 1)),
                                background=self.ckpt_background,
                                _after=lambda: TS.prune(ckpt_dir, keep))
            if callback is not None:
                callback(entry)
