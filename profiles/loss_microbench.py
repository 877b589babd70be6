"""Solo timing of the loss kernels at a given image size, planar [3,H,W] and interleaved [H,W,3] layouts
(python profiles/loss_microbench.py [W H]); CLMGS_LIB_PATH selects a library build.  The unmasked pair and the masked
pair (clmgs_l1_ssim_loss_masked_fwd/_bwd, a half-counted mask) come out of the same library and are timed alternately,
ROUNDS windows of REPS launches each; the median and the fastest window are printed per kernel."""
import statistics
import sys
import torch
sys.path.insert(0, ".")
from clm_gs_amd import _lib
from clm_gs_amd._lib import check, dptr, stream
W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4608, 3456)
ROUNDS, REPS = 5, 20
L = _lib.lib()
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
base = torch.rand((3, H, W), device=dev, generator=g)
gt = (torch.rand((3, H, W), device=dev, generator=g) * 255).to(torch.uint8)
# half of the pixels counted, two ways: 256-pixel blocks in a checkerboard (what a segmentation looks like to a 64-lane
# strip: long runs), and independent coin flips (every wavefront mixed)
yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
MASKS = {"blocks": ((((yy // 256) + (xx // 256)) % 2) * 255).to(torch.uint8).contiguous(),
         "coins": (torch.rand((H, W), device=dev, generator=g) < 0.5).to(torch.uint8).contiguous()}
del yy, xx
maps = torch.empty((3, 3, H, W), device=dev)
one = torch.ones(1, device=dev)
U8 = torch.uint8
res = {}
for name in ("planar", "interleaved"):
    if name == "planar":
        img = base.clone(); sc, sy, sx = H * W, W, 1
    else:
        img = base.permute(1, 2, 0).contiguous(); sc, sy, sx = 1, 3 * W, 3
    v_img = torch.empty_like(img)
    part = torch.zeros((L.clmgs_loss_slots(), 2), device=dev)
    mask = None
    def fwd():
        check(L.clmgs_l1_ssim_loss_fwd(stream(), H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(part),
                                       dptr(maps[0]), dptr(maps[1]), dptr(maps[2])))
    def bwd():
        check(L.clmgs_l1_ssim_loss_bwd(stream(), H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(one), 0.2,
                                       dptr(maps[0]), dptr(maps[1]), dptr(maps[2]), dptr(v_img)))
    def mfwd():
        check(L.clmgs_l1_ssim_loss_masked_fwd(stream(), H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(part),
                                              dptr(maps[0]), dptr(maps[1]), dptr(maps[2]), dptr(mask, U8)))
    def mbwd():
        check(L.clmgs_l1_ssim_loss_masked_bwd(stream(), H, W, dptr(img), sc, sy, sx, dptr(gt, U8), dptr(one), 0.2,
                                              dptr(maps[0]), dptr(maps[1]), dptr(maps[2]), dptr(v_img), dptr(mask, U8)))
    def window(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / REPS
    kernels = [("fwd", fwd, None), ("bwd", bwd, None)]
    for mname in MASKS:
        kernels += [(f"masked_{mname}_fwd", mfwd, mname), (f"masked_{mname}_bwd", mbwd, mname)]
    times = {k: [] for k, _, _ in kernels}
    for rnd in range(ROUNDS + 1):  # round 0 warms every kernel up
        for k, f, mname in kernels:
            mask = MASKS[mname] if mname else None
            if rnd == 0:
                for _ in range(3):
                    f()
                torch.cuda.synchronize()
            else:
                times[k].append(window(f))
    for k, t in times.items():
        res[f"{name}_{k}_ms"] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4)}
    for k in ("fwd", "bwd"):
        for mname in MASKS:
            res[f"{name}_masked_{mname}_{k}_over_unmasked"] = round(
                res[f"{name}_masked_{mname}_{k}_ms"]["median"] / res[f"{name}_{k}_ms"]["median"], 4)
    # results of the last pair run (masked, "coins"), as a sanity check that the kernels did their work
    part.zero_()
    mask = MASKS["coins"]
    mfwd(); mbwd()
    res[f"{name}_masked_coins_sums_per_value"] = (part.sum(0) / (3.0 * H * W)).tolist()
    res[f"{name}_masked_coins_vsum"] = float(v_img.double().abs().sum())
for k, v in res.items():
    print(k, v)
