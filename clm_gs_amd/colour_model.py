"""What exposure.ExposureModel and bilagrid.BilagridModel share: one learnable table with a row per training camera, a
gradient table the kernels ADD into, the cameras' views of both (cameras.camera_colour reads them), and a dense Adam step
at a scheduled learning rate.  The optimizer, the schedule and the file formats belong to the subclass.  sky.SkyModel
builds on the same base with ONE table for the scene (its own attach) and a fixed-point accumulator in front of `grad`."""
import torch


class ColourModel:
    KIND = None  # "exposure" | "bilagrid": a camera carries `<KIND>` and `<KIND>_grad`

    def __init__(self, table):
        """table: float32 [n_cameras, ...] on the model's device.  The subclass sets `optimizer` and `lr_func` afterwards."""
        self.n_cameras = int(table.shape[0])
        # the leaf the optimizer steps; cameras get views of its storage that carry no autograd history
        self.param = table.contiguous().requires_grad_(True)
        self.grad = torch.zeros_like(self.param)
        self.param.grad = self.grad  # the kernels ADD into rows of this table; zero_grad() clears it in place

    def attach(self, cameras):
        """camera i of the list trains row i: `camera.<KIND>` / `camera.<KIND>_grad` are VIEWS of the tables."""
        assert len(cameras) == self.n_cameras, (len(cameras), self.n_cameras)
        rows = self.param.detach()
        for i, c in enumerate(cameras):
            setattr(c, self.KIND, rows[i])
            setattr(c, self.KIND + "_grad", self.grad[i])

    def before_step(self):
        """What a subclass adds into `grad` before the optimizer steps (a regulariser's gradient)."""

    def step(self, iteration):
        """before_step(), then one Adam step at the scheduled learning rate; enqueued on the current stream, which must be
        ordered after the streams the cameras' gradient kernels ran on (the engines join them at the end of a batch)."""
        lr = float(self.lr_func(iteration))
        for group in self.optimizer.param_groups:
            group["lr"] = lr
        if self.param.grad is not self.grad:
            self.param.grad = self.grad
        self.before_step()
        self.optimizer.step()
        return lr

    def zero_grad(self):
        self.grad.zero_()

    # ---- the trainer's calls on every side model, pose.PoseModel too; save_to(model_dir, cameras) writes the subclass's FILE
    def end_batch(self, iteration, batch_cameras):
        self.step(iteration)
        self.zero_grad()

    def flush(self):
        """Nothing is deferred: a step is enqueued when it is asked for."""
