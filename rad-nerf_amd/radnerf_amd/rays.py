"""Ray generation for a training batch (first half):
datasets/ray_utils.py:45-70 (get_rays) and the per-batch pose / pixel gather
of train_ml.py:84-96 as one HIP pass (rn_get_rays); with per-image pose
refinement (--optimize_ext, train_ml.py:90-93) rn_get_rays_pose and its
backward into dR / dT (rn_get_rays_pose_bw)."""
import torch

from ._lib import lib


def _c(t, dtype=torch.float32):
    return t.to(dtype).contiguous()


def get_rays(directions, c2w):
    """ray_utils.get_rays: directions (N,3), c2w (3,4) or (N,3,4) -> rays_o, rays_d."""
    directions = _c(directions)
    n = directions.shape[0]
    dev = directions.device
    rays_o = torch.empty(n, 3, device=dev)
    rays_d = torch.empty(n, 3, device=dev)
    c2w = _c(c2w)
    img = None
    if c2w.ndim == 3:
        img = torch.arange(n, device=dev, dtype=torch.int64)
    lib().get_rays(directions.data_ptr(), c2w.data_ptr(), None if img is None else img.data_ptr(),
                   None, n, None, rays_o.data_ptr(), rays_d.data_ptr(), None,
                   torch.cuda.current_stream(dev).cuda_stream)
    return rays_o, rays_d


def batch_rays(directions, poses, img_idxs, pix_idxs, with_imgs_d=True):
    """train_ml.py:84-96 for split='train': rays_o, rays_d (and imgs_d, the
    pose applied to the mean camera direction) of the picked pixels."""
    directions, poses = _c(directions), _c(poses)
    img_idxs, pix_idxs = _c(img_idxs, torch.int64), _c(pix_idxs, torch.int64)
    n = img_idxs.shape[0]
    dev = directions.device
    rays_o = torch.empty(n, 3, device=dev)
    rays_d = torch.empty(n, 3, device=dev)
    imgs_d = torch.empty(n, 3, device=dev) if with_imgs_d else None
    mean_dir = directions.mean(0).contiguous() if with_imgs_d else None
    lib().get_rays(directions.data_ptr(), poses.data_ptr(), img_idxs.data_ptr(),
                   pix_idxs.data_ptr(), n, None if mean_dir is None else mean_dir.data_ptr(),
                   rays_o.data_ptr(), rays_d.data_ptr(),
                   None if imgs_d is None else imgs_d.data_ptr(),
                   torch.cuda.current_stream(dev).cuda_stream)
    return (rays_o, rays_d, imgs_d) if with_imgs_d else (rays_o, rays_d)


def _check_pose_args(directions, poses, dR, dT, img_idxs, pix_idxs):
    """Shape / dtype checks of pose_rays (no device needed)."""
    if directions.ndim != 2 or directions.shape[1] != 3:
        raise ValueError(f"pose_rays: directions must be (P, 3), got {tuple(directions.shape)}")
    if poses.ndim != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"pose_rays: poses must be (N, 3, 4), got {tuple(poses.shape)}")
    n = poses.shape[0]
    for name, t in (("dR", dR), ("dT", dT)):
        if t is not None and tuple(t.shape) != (n, 3):
            raise ValueError(f"pose_rays: {name} must be ({n}, 3) for {n} poses, got "
                             f"{tuple(t.shape)}")
    for name, t in (("img_idxs", img_idxs), ("pix_idxs", pix_idxs)):
        if t.ndim != 1 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError(f"pose_rays: {name} must be a 1-D integer tensor")
    if img_idxs.shape[0] != pix_idxs.shape[0]:
        raise ValueError(f"pose_rays: {img_idxs.shape[0]} img_idxs vs {pix_idxs.shape[0]} "
                         "pix_idxs")


def pose_rays_backward(directions, poses, dR, img_idxs, pix_idxs, mean_dir, g_o, g_d, g_i,
                       out_dR, out_dT):
    """rn_get_rays_pose_bw into out_dR / out_dT ((N, 3) fp32 contiguous, e.g.
    views of a flat gradient buffer): every row is written, nothing is
    accumulated.  All tensors are what pose_rays' forward was given (fp32 /
    int64, contiguous); g_i and mean_dir may be None together."""
    n_img = poses.shape[0]
    for t in (out_dR, out_dT):
        if not (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n_img, 3)):
            raise ValueError(f"pose_rays_backward: outputs must be contiguous fp32 ({n_img}, 3)")
    lib().get_rays_pose_bw(directions.data_ptr(), poses.data_ptr(),
                           None if dR is None else dR.data_ptr(), img_idxs.data_ptr(),
                           pix_idxs.data_ptr(), img_idxs.shape[0], n_img,
                           None if g_i is None else mean_dir.data_ptr(), g_o.data_ptr(),
                           g_d.data_ptr(), None if g_i is None else g_i.data_ptr(),
                           out_dR.data_ptr(), out_dT.data_ptr(),
                           torch.cuda.current_stream(directions.device).cuda_stream)
    return out_dR, out_dT


class _PoseRaysFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dR, dT, directions, poses, img_idxs, pix_idxs, mean_dir):
        n = img_idxs.shape[0]
        dev = directions.device
        rays_o = torch.empty(n, 3, device=dev)
        rays_d = torch.empty(n, 3, device=dev)
        imgs_d = None if mean_dir is None else torch.empty(n, 3, device=dev)
        lib().get_rays_pose(directions.data_ptr(), poses.data_ptr(), dR.data_ptr(),
                            dT.data_ptr(), img_idxs.data_ptr(), pix_idxs.data_ptr(), n,
                            None if mean_dir is None else mean_dir.data_ptr(),
                            rays_o.data_ptr(), rays_d.data_ptr(),
                            None if imgs_d is None else imgs_d.data_ptr(),
                            torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(dR, directions, poses, img_idxs, pix_idxs, mean_dir)
        if imgs_d is None:
            return rays_o, rays_d
        return rays_o, rays_d, imgs_d

    @staticmethod
    def backward(ctx, g_o, g_d, g_i=None):
        dR, directions, poses, img_idxs, pix_idxs, mean_dir = ctx.saved_tensors
        n, dev = img_idxs.shape[0], directions.device
        g_o = torch.zeros(n, 3, device=dev) if g_o is None else _c(g_o)
        g_d = torch.zeros(n, 3, device=dev) if g_d is None else _c(g_d)
        g_i = None if g_i is None else _c(g_i)
        out_dR, out_dT = torch.empty_like(dR), torch.empty_like(dR)
        pose_rays_backward(directions, poses, dR, img_idxs, pix_idxs, mean_dir, g_o, g_d, g_i,
                           out_dR, out_dT)
        return out_dR, out_dT, None, None, None, None, None


def pose_rays(directions, poses, dR, dT, img_idxs, pix_idxs, with_imgs_d=True, mean_dir=None):
    """batch_rays with the per-image pose refinement of --optimize_ext
    (train_ml.py:90-93): poses[n] rotated by the axis-angle dR[n] and shifted by
    dT[n] ((N, 3) each) before the rays are formed.  Differentiable in dR and
    dT only (directions and poses are data and get no gradient); zero dR / dT
    give batch_rays' rays.  mean_dir: directions.mean(0) when the caller keeps
    it (it is recomputed per call otherwise)."""
    _check_pose_args(directions, poses, dR, dT, img_idxs, pix_idxs)
    directions, poses = _c(directions.detach()), _c(poses.detach())
    dR, dT = _c(dR), _c(dT)
    img_idxs, pix_idxs = _c(img_idxs, torch.int64), _c(pix_idxs, torch.int64)
    if with_imgs_d:
        mean_dir = directions.mean(0).contiguous() if mean_dir is None else _c(mean_dir.detach())
    else:
        mean_dir = None
    return _PoseRaysFn.apply(dR, dT, directions, poses, img_idxs, pix_idxs, mean_dir)
