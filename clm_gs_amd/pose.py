"""Camera pose refinement: one learnable rigid correction per training camera (gsplat's `pose_opt` /
CameraOptModule; DESIGN.md section 3, "Pose refinement").  Row i of the table is  dx (3) | d6 (6), zero at the start, and

    c2w_i = c2w0_i . [ rot6d(d6 + (1,0,0,0,1,0)) | dx ]        (Zhou et al.'s 6-D rotation, as gsplat)

The gradient of the loss with respect to a camera is produced by the kernels of csrc/pose.hip as 15 floats
(v_R 9 | v_t 3 | v_campos 3: the cotangents of the world-to-camera matrix and of the camera centre, kept apart);
fused.camera_backward launches them for a camera that carries a buffer (`attach`).  This module composes the 15
floats into the gradient of the row by autograd through  viewmat = inverse(c2w), campos = c2w[:3, 3],  steps the table
with dense Adam + weight decay, and writes the moved cameras back.

Everything here lives on the HOST in float64: the table is a few thousand rows and the kernels take the camera
matrices from the host by value.  The gradients travel as the trainer's loss values do (pinned buffer, side stream,
event), and by default the step of batch b is applied once batch b+1 has been enqueued, so the host never drains the
device (`defer_pose_step`).  What that delays: batch b+1 is rendered at the poses BEFORE step b.  A camera of batch
b+1 that was also in batch b (possible only where an epoch ends and the next shuffle begins) therefore sees a pose
that misses its own newest gradient; every other camera of batch b+1 misses only step b's momentum and weight-decay
tail of its earlier gradients.  `defer_pose_step=False` applies the step immediately (the host then waits for the
batch): the sequential semantics."""
import json
import math
import os

import numpy as np
import torch

from . import dp

F64 = torch.float64
_I6 = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def rot6d_to_matrix(d6):
    """[..., 6] -> [..., 3, 3]: Gram-Schmidt on the two 3-vectors, the third row their cross product (rows b1, b2, b3)."""
    a1, a2 = d6[..., :3], d6[..., 3:]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    b2 = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = b2 / b2.norm(dim=-1, keepdim=True)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def compose_c2w(c2w0, rows):
    """c2w0 [n,4,4], rows [n,9] (dx | d6) -> c2w [n,4,4] = c2w0 @ [rot6d(d6 + I6) | dx]."""
    n = rows.shape[0]
    rot = rot6d_to_matrix(rows[:, 3:] + rows.new_tensor(_I6))
    top = torch.cat((rot, rows[:, :3, None]), dim=2)
    bottom = rows.new_tensor((0.0, 0.0, 0.0, 1.0)).expand(n, 1, 4)
    return c2w0 @ torch.cat((top, bottom), dim=1)


def check_pose_args(args, depth_priors=False, enabled=None):
    """Pose refinement runs on clm_offload with the SH rows in HBM and on no_offload, both through the fused front end,
    on one GPU; every other combination is refused here by name, before anything is loaded."""
    if not (bool(getattr(args, "pose_opt", False)) if enabled is None else enabled):
        return
    why = None
    if bool(getattr(args, "naive_offload", False)):
        why = "naive_offload: its engine does not run the fused front end that produces the camera gradient"
    elif not bool(getattr(args, "fused_front_end", True)):
        why = "fused_front_end=False: the camera gradient is a kernel of the fused front end (the op-by-op route has " \
              "gsplat.fully_fused_projection(viewmats.requires_grad_()) instead)"
    elif getattr(args, "sh_residency", "hbm") == "host":
        why = 'sh_residency="host": the pose kernel reads the SH rows from HBM'
    elif float(getattr(args, "sh_hbm_budget_gb", 0.0) or 0.0) > 0.0:
        why = "sh_hbm_budget_gb > 0: the HBM-resident prefix belongs to the host-resident mode"
    elif dp.world_size() > 1:
        why = dp.refusal(dp.world_size(), "the pose table is not reduced")
    elif depth_priors or bool(getattr(args, "depths", "")):
        why = "--depths / depth render modes: the fourth channel's cotangent reaches the positions outside the " \
              "projection VJP, and the camera gradient would miss it"
    if why:
        raise ValueError("pose_opt is not supported with " + why)


class PoseModel:
    """gsplat's CameraOptModule + its Adam, on the host in float64."""
    FILE = "poses.json"  # {image_name: {"delta": [9], "world_to_camera": 4x4}}

    def __init__(self, n_cameras, lr=1e-5, reg=1e-6, max_steps=30000, defer=True, device="cuda", lr_final_factor=0.01,
                 betas=(0.9, 0.999), eps=1e-8):
        self.n_cameras = int(n_cameras)
        self.table = torch.zeros((self.n_cameras, 9), dtype=F64)
        self.exp_avg = torch.zeros_like(self.table)
        self.exp_avg_sq = torch.zeros_like(self.table)
        self.t = 0                      # Adam steps taken
        self.lr, self.reg, self.max_steps = float(lr), float(reg), max(int(max_steps), 1)
        self.lr_final_factor, self.betas, self.eps = float(lr_final_factor), (float(betas[0]), float(betas[1])), float(eps)
        self.defer = bool(defer)
        self.device = device
        self.cameras = None
        self.c2w0 = None                # [n,4,4] float64: the poses as loaded
        self._applied = torch.zeros_like(self.table)  # the rows the cameras' fields currently reflect
        self.grad = None                # [n,16] float32 on the device: row i is camera i's 15-float buffer (+ pad)
        self._index = {}
        self._pending, self._stream, self._hosts, self._turn = None, None, {}, 0

    # ---- cameras
    def attach(self, cameras):
        """Camera i of the list trains row i and receives its gradient buffer (`camera.pose_grad`, 15 floats the kernels
        ADD into).  Without a device (host-only use: tests, tools) no buffer is made."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        self.cameras = list(cameras)
        w2c = torch.stack([torch.from_numpy(np.asarray(c._clmgs_host[0], dtype=np.float64).reshape(4, 4).copy())
                           if getattr(c, "_clmgs_host", None) is not None
                           else c.world_view_transform.detach().t().cpu().to(F64) for c in cameras])
        self.c2w0 = torch.inverse(w2c)
        self._index = {id(c): i for i, c in enumerate(cameras)}
        if self.device is not None and torch.cuda.is_available():
            self.grad = torch.zeros((self.n_cameras, 16), dtype=torch.float32, device=self.device)
            for i, c in enumerate(cameras):
                c.pose_grad = self.grad[i, :15]
        self.refresh()

    def perturb(self, noise, seed=0):
        """gsplat's pose_noise: a seeded normal perturbation of the whole table (std `noise`), for experiments."""
        g = torch.Generator().manual_seed(int(seed))
        self.table += torch.randn(self.table.shape, generator=g, dtype=F64) * float(noise)
        self.refresh()

    def camtoworlds(self, rows=None):
        """float64 [n,4,4] camera-to-world matrices of the current table (or of `rows`)."""
        return compose_c2w(self.c2w0, self.table if rows is None else rows)

    def refresh(self):
        """Writes every camera whose row differs from what its fields reflect: world_view_transform, camtoworlds and the
        cached host triple, all from the same float64 matrix.  A camera whose row has not moved is not touched (a zero
        table leaves the cameras as loaded, bit for bit).  -> the number of cameras written."""
        if self.cameras is None:
            return 0
        moved = torch.nonzero((self.table != self._applied).any(dim=1)).flatten().tolist()
        if not moved:
            return 0
        c2w = compose_c2w(self.c2w0[moved], self.table[moved])
        w2c = torch.inverse(c2w)
        # [m,2,4,4] float32: the TRANSPOSED world-to-camera matrix (world_view_transform's layout) | camera-to-world
        pair = torch.stack((w2c.transpose(1, 2), c2w), dim=1).to(torch.float32).contiguous()
        w32 = w2c.to(torch.float32).numpy().reshape(-1, 16).copy()
        centre = pair[:, 1, :3, 3].numpy().copy()
        # ONE upload per device for all moved cameras, from pinned memory: enqueued, never waited for
        on_dev = {}
        for dev in {self.cameras[i].world_view_transform.device for i in moved}:
            on_dev[dev] = pair.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else pair.clone()
        for j, i in enumerate(moved):
            cam = self.cameras[i]
            up = on_dev[cam.world_view_transform.device]
            cam.world_view_transform = up[j, 0]
            cam.camtoworlds = up[j, 1][None]
            old = getattr(cam, "_clmgs_host", None)
            K = old[1] if old is not None else np.ascontiguousarray(
                cam.create_k_on_gpu("cpu").numpy().astype(np.float32).reshape(9))
            # a NEW triple (rows of fresh arrays): a camera pass in flight keeps the one it was enqueued with
            cam._clmgs_host = (w32[j], K, centre[j])
        self._applied[moved] = self.table[moved]
        return len(moved)

    # ---- gradient
    def compose_grad(self, ids, g15):
        """ids: camera indices [b]; g15 [b,15] (v_R | v_t | v_campos).  -> float64 [b,9], the gradient of the rows: autograd
        of  <v_R, viewmat[:3,:3]> + <v_t, viewmat[:3,3]> + <v_campos, campos>  through viewmat = inverse(c2w),
        campos = c2w[:3,3], c2w = compose_c2w(c2w0, row)."""
        g15 = torch.as_tensor(g15).to(F64).reshape(len(ids), 15)
        rows = self.table[ids].clone().requires_grad_(True)
        c2w = compose_c2w(self.c2w0[ids], rows)
        vm = torch.inverse(c2w)
        s = (g15[:, :9].reshape(-1, 3, 3) * vm[:, :3, :3]).sum() + (g15[:, 9:12] * vm[:, :3, 3]).sum() \
            + (g15[:, 12:15] * c2w[:, :3, 3]).sum()
        return torch.autograd.grad(s, rows)[0]

    def learning_rate(self, t):
        """lr * lr_final_factor^(t / max_steps) for the 0-based count t of steps already taken (gsplat's ExponentialLR with
        gamma = 0.01^(1/max_steps))."""
        return self.lr * self.lr_final_factor ** (min(int(t), self.max_steps) / self.max_steps)

    def apply(self, ids, g15):
        """One dense Adam step (weight decay `reg` added to the gradient, torch.optim.Adam's form) of the WHOLE table with
        the composed gradient of cameras `ids` (a camera listed twice adds up), then refresh()."""
        grad = torch.zeros_like(self.table)
        if len(ids):
            grad.index_add_(0, torch.as_tensor(list(ids), dtype=torch.int64), self.compose_grad(list(ids), g15))
        b1, b2 = self.betas
        lr = self.learning_rate(self.t)
        self.t += 1
        g = grad + self.reg * self.table
        self.exp_avg.mul_(b1).add_(g, alpha=1.0 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1.0 - b2)
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(1.0 - b2 ** self.t)).add_(self.eps)
        self.table.addcdiv_(self.exp_avg, denom, value=-lr / (1.0 - b1 ** self.t))
        self.refresh()
        return lr

    # ---- the trainer's call, once per batch, after the engine has enqueued it
    def step(self, batch_cameras, g15=None):
        """Takes the gradients of the batch's cameras off the device (or `g15` [b,15], host values: tests) and steps.
        Deferred (default): the copy travels on a side stream behind an event and the step of the PREVIOUS call is
        applied now; flush() applies the last one.  Immediate: waits for the copy and steps."""
        ids = [self._index[id(c)] for c in batch_cameras]
        if g15 is not None:
            item = (ids, torch.as_tensor(g15).to(F64).reshape(len(ids), 15).clone(), None)
        else:
            item = self._collect(ids)
        if not self.defer:
            self._apply_item(item)
            return
        prev, self._pending = self._pending, item
        if prev is not None:
            self._apply_item(prev)

    def end_batch(self, iteration, batch_cameras):
        self.step(batch_cameras)

    def flush(self):
        if self._pending is not None:
            item, self._pending = self._pending, None
            self._apply_item(item)

    def _collect(self, ids):
        if self._stream is None:
            self._stream = torch.cuda.Stream()
        cur = torch.cuda.current_stream()
        # behind the batch on the current stream, which the engines joined (views of the table: no index upload)
        stacked = torch.stack([self.grad[i] for i in ids])
        for i in set(ids):
            self.grad[i].zero_()  # the rows start the next batch at zero
        ev = torch.cuda.Event()
        ev.record(cur)
        self._turn ^= 1
        key = (len(ids), self._turn)  # two pinned buffers per batch size, used alternately
        host = self._hosts.get(key)
        if host is None:
            host = self._hosts[key] = torch.empty((len(ids), 16), dtype=torch.float32, pin_memory=True)
        with torch.cuda.stream(self._stream):
            self._stream.wait_event(ev)
            host.copy_(stacked, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._stream)
        stacked.record_stream(self._stream)
        return ids, host, done

    def _apply_item(self, item):
        ids, host, done = item
        if done is not None:
            done.synchronize()
        self.apply(ids, host[:, :15])

    # ---- files
    def save_json(self, path, cameras):
        """{image_name: {"delta": [9], "world_to_camera": 4x4}} of the current table (a float64 survives its repr)."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        w2c = torch.inverse(self.camtoworlds())
        with open(path, "w") as f:
            json.dump({c.image_name: {"delta": self.table[i].tolist(), "world_to_camera": w2c[i].tolist()}
                       for i, c in enumerate(cameras)}, f, indent=2)

    def save_to(self, model_dir, cameras):
        self.save_json(os.path.join(model_dir, self.FILE), cameras)

    def load_json(self, path, cameras):
        """Rows of the cameras named in the file (a camera the file does not name keeps its row), then refresh()."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        with open(path) as f:
            table = json.load(f)
        for i, c in enumerate(cameras):
            if c.image_name in table:
                row = torch.tensor(table[c.image_name]["delta"], dtype=F64)
                if tuple(row.shape) != (9,):
                    raise ValueError(f"{path}: delta of {c.image_name} is {tuple(row.shape)}, not [9]")
                self.table[i] = row
        self.refresh()
        return table
