"""-m gpu: the resolution schedule ("Resolution schedule") -- the three entries of csrc/resample.hip
against the integer reference (tests/resample_reference.py) bit for bit, the operator's `out=`, the alignment of a level
view with the resampled ground truth, and the trainer's schedule in every engine."""
import functools
import io
import re

import numpy as np
import pytest
import torch

from tests import resample_reference as R

pytestmark = pytest.mark.gpu

LEVELS = [1, 2]
# (H, W): one pixel, smaller than a cell, odd, no multiple of the cell, exact, just past exact, more than one workgroup
# in y / more than one wave step in x, and the two long thin ones that cross workgroup and vector-width edges
SIZES = [(1, 1), (2, 2), (3, 5), (7, 9), (16, 16), (17, 33), (65, 47), (5, 1031), (1031, 5)]
FULL = (3456, 4608)


def _ids(v):
    return f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _inputs(kind, hw, fill):
    """(input array, {level: expected}) -- computed once, shared, never written to."""
    H, W = hw
    rng = np.random.default_rng(H * 10007 + W)
    if kind == "u8":
        top, shape, dtype = 255, (3, H, W), np.uint8      # three planes whose contents differ
    elif kind == "u16":
        top, shape, dtype = 65535, (H, W), np.uint16
    if kind in ("u8", "u16"):
        a = {"random": lambda: rng.integers(0, top + 1, size=shape), "zero": lambda: np.zeros(shape),
             "max": lambda: np.full(shape, top)}[fill]().astype(dtype)
        a.setflags(write=False)
        return a, {L: R.area_resample(a, L) for L in LEVELS}
    m = (rng.random((H, W)) < float(fill)) * rng.integers(1, 256, size=(H, W))   # counted pixels carry any non-zero byte
    m = m.astype(np.uint8)
    m.setflags(write=False)
    return m, {L: R.mask_resample(m, L) for L in LEVELS}


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


@pytest.mark.parametrize("fill", ["random", "zero", "max"])
@pytest.mark.parametrize("hw", SIZES, ids=_ids)
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_entries_match_the_reference_bit_for_bit(dev, kind, hw, fill):
    from clm_gs_amd import clm_kernels as K
    a, want = _inputs(kind, hw, fill)
    t = _dev(a, dev)
    for L in LEVELS:
        got = K.area_resample(t, L)
        assert got.dtype == t.dtype and tuple(got.shape) == want[L].shape
        got = got.cpu().numpy()
        assert np.array_equal(got, want[L]), (L, np.argwhere(got != want[L])[:5], got.ravel()[:8], want[L].ravel()[:8])
    if kind == "u8":  # one plane alone, as a [H,W] tensor
        assert np.array_equal(K.area_resample(t[1].contiguous(), 1).cpu().numpy(), want[1][1])


@pytest.mark.parametrize("density", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("hw", SIZES, ids=_ids)
def test_mask_entry_and_its_count(dev, hw, density):
    from clm_gs_amd import clm_kernels as K
    m, want = _inputs("mask", hw, density)
    t = _dev(m, dev)
    for L in LEVELS:
        got, count = K.area_resample(t, L, mask=True)
        assert count.dtype == torch.int64 and tuple(count.shape) == (1,)
        assert np.array_equal(got.cpu().numpy(), want[L][0]), (L, hw, density)
        assert int(count.item()) == want[L][1] == int(np.count_nonzero(want[L][0]))


@pytest.mark.parametrize("kind", ["u8", "u16", "mask"])
def test_full_size_all_max_stays_all_max(dev, kind):
    """3456 x 4608 at level 2: S = W H 255 (or 65535) passes 2^32; the expected value needs no CPU resampling."""
    from clm_gs_amd import clm_kernels as K
    H, W = FULL
    Ho, Wo = R.level_size(H, W, 2)
    if kind == "u8":
        out = K.area_resample(torch.full((3, H, W), 255, dtype=torch.uint8, device=dev), 2)
        assert tuple(out.shape) == (3, Ho, Wo) and bool((out == 255).all())
    elif kind == "u16":
        out = K.area_resample(torch.full((H, W), 65535, dtype=torch.uint16, device=dev), 2)
        assert tuple(out.shape) == (Ho, Wo) and bool((out.to(torch.int32) == 65535).all())
    else:
        out, count = K.area_resample(torch.full((H, W), 255, dtype=torch.uint8, device=dev), 2, mask=True)
        assert tuple(out.shape) == (Ho, Wo) and bool((out == 255).all()) and int(count.item()) == Ho * Wo


def test_out_writes_the_given_buffer_and_allocates_nothing(dev):
    from clm_gs_amd import _lib, clm_kernels as K
    a, want = _inputs("u8", (65, 47), "random")
    t = _dev(a, dev)
    buf = torch.zeros((3,) + R.level_size(65, 47, 1), dtype=torch.uint8, device=dev)
    K.area_resample(t, 1, out=buf)  # (the first call loads the code object)
    buf.zero_()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    ret = K.area_resample(t, 1, out=buf)
    after = torch.cuda.memory_allocated()
    assert ret is buf and before == after
    assert np.array_equal(buf.cpu().numpy(), want[1])
    assert K.area_resample(t, 0) is t  # level 0: the input itself, no kernel
    with pytest.raises(_lib.ClmgsError):
        K.area_resample(t, 1, out=torch.zeros((3, 5, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(_lib.ClmgsError):
        K.area_resample(t.float(), 1)
    with pytest.raises(_lib.ClmgsError):
        K.area_resample(t, 9)  # f = 512: past what a wave's columns hold; refused by the entry, nothing launched


# ------------------------------------------------------------------------------------------------- model, cameras
N, W, H, BSZ = 3000, 96, 64, 4
N_CAMS = 12


def _psnr(a, b):
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


def _truth_model(dev):
    from clm_gs_amd import utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload
    from clm_gs_amd.synthetic import synth_gaussians
    truth = synth_gaussians(N, seed=7, device="cuda")
    model = GaussianModelCLMOffload(3, only_for_rendering=True)
    model.args = utils.default_args(bsz=BSZ, sh_residency="hbm")
    model.create_from_tensors(truth["xyz"], truth["shs48"], truth["scaling"], truth["rotation"], truth["opacity"])
    model.active_sh_degree = 3
    return truth, model


def _render_with_K(truth, model, camera, K):
    """The op-by-op forward of all rows with the camera's pose and the K handed in, at the global image size."""
    from clm_gs_amd.strategies.base_engine import camera_forward_ops
    with torch.no_grad():
        viewmat = camera.world_view_transform.transpose(0, 1)
        centre = torch.inverse(viewmat.unsqueeze(0))[:, None, :3, 3]
        image = camera_forward_ops(truth["xyz"], model.rotation_activation(truth["rotation"]),
                                   model.scaling_activation(truth["scaling"]), model.opacity_activation(truth["opacity"]),
                                   truth["shs48"].reshape(1, N, 16, 3), 3, viewmat, K, centre, None, "RGB", train=False)[0]
    return image.clamp(0, 1)


def test_a_level_view_is_aligned_with_the_resampled_ground_truth(dev):
    """Relational, no threshold: the level-1 render agrees better with the area-resampled full-size render than the same
    view with its principal point moved by half a level pixel does.  (The evaluation entry builds its K from the FoV and
    the global size, so the moved principal point goes through the op-by-op forward, which takes a K -- and the view's own
    K goes through it too.)"""
    from clm_gs_amd import cameras, clm_kernels as K, utils
    from clm_gs_amd.strategies.clm_offload import clm_offload_eval_one_cam
    from clm_gs_amd.synthetic import nadir_cameras
    utils.set_args(utils.default_args(bsz=BSZ, clm_offload=True))
    utils.set_cur_iter(1)
    truth, model = _truth_model(dev)
    cam = nadir_cameras(4, N, W, H, 0.3, seed=7, device="cuda")[1]
    try:
        utils.set_img_size(H, W)
        full = clm_offload_eval_one_cam(cam, model, None, None).clamp(0, 1)
        gt = (full * 255).round().to(torch.uint8).contiguous()
        level_gt = K.area_resample(gt, 1).float() / 255.0
        view = cameras.level_view(cam, 1)
        utils.set_img_size(view.image_height, view.image_width)
        aligned = _psnr(clm_offload_eval_one_cam(view, model, None, None).clamp(0, 1), level_gt)
        own_K = _psnr(_render_with_K(truth, model, view, view.K), level_gt)
        moved_K = view.K.clone()
        moved_K[0, 2] += 0.5
        moved_K[1, 2] += 0.5
        moved = _psnr(_render_with_K(truth, model, view, moved_K), level_gt)
    finally:
        utils.set_img_size(H, W)
    print(f"level-1 view against the resampled ground truth: PSNR {aligned:.2f} dB (evaluation entry), {own_K:.2f} dB "
          f"(the view's K); principal point moved by half a level pixel: {moved:.2f} dB")
    assert aligned > moved and own_K > moved, (aligned, own_K, moved)


# ------------------------------------------------------------------------------------------------------- trainer
D, SCHEDULE, IMAGES = 2, 8, 32
LEVEL_LINE = re.compile(r"^resolution level (\d+): (\d+)x(\d+) from iteration (\d+)$", re.M)
ROUND = 512  # the caching allocator's granularity: what a tensor of n bytes adds to memory_allocated is n rounded up to it


def _alloc(n_bytes):
    return -(-int(n_bytes) // ROUND) * ROUND


def _train(monkeypatch, strategy, residency, variant=None, num_downscales=D, explicit=True, break_mask=False,
           keep_params=False):
    """One run of training(...) on cameras as objects -> a dict of what the tests look at."""
    from clm_gs_amd import trainer, utils
    from clm_gs_amd.strategies.clm_offload import GaussianModelCLMOffload, clm_offload_eval_one_cam
    from clm_gs_amd.strategies.naive_offload import GaussianModelNaiveOffload
    from clm_gs_amd.strategies.no_offload import GaussianModelNoOffload
    from clm_gs_amd.synthetic import nadir_cameras
    over = dict(num_downscales=num_downscales, resolution_schedule=SCHEDULE) if explicit else {}
    args = utils.default_args(bsz=BSZ, sh_residency=residency, **over)
    setattr(args, strategy, True)
    utils.set_args(args)
    utils.set_img_size(H, W)
    utils.set_cur_iter(1)
    truth, gt_model = _truth_model("cuda")
    cams = nadir_cameras(N_CAMS, N, W, H, 0.3, seed=7, device="cuda")
    for c in cams:
        c.original_image = (clm_offload_eval_one_cam(c, gt_model, None, None).clamp(0, 1) * 255).round().to(torch.uint8)
    g = torch.Generator(device="cuda").manual_seed(1)
    extra_bytes = 0
    Hs, Ws = R.level_size(H, W, D)  # the coarsest level: where the peak of the coarse phase is asked about
    if variant == "mask":
        for c in cams[:2]:
            m = (torch.rand((H, W), generator=g, device="cuda") < 0.7).to(torch.uint8)
            c.loss_mask, c.loss_mask_count = m, int(m.count_nonzero())
        extra_bytes += 2 * _alloc(Hs * Ws) + _alloc(2 * 8)   # two level masks, their two counts
    if variant == "depth":
        for c in cams[:2]:
            c.invdepth = (torch.rand((H, W), generator=g, device="cuda") * 20000 + 20000).to(torch.int32).to(torch.uint16)
            c.invdepth_scale, c.invdepth_offset = 1.0, 0.0
        extra_bytes += 2 * _alloc(Hs * Ws * 2) + _alloc(8)
    if break_mask:
        cams[0].loss_mask = torch.ones((H + 2, W), dtype=torch.uint8, device="cuda")
        cams[0].loss_mask_count = (H + 2) * W
    noisy_sh = truth["shs48"].clone()
    noisy_sh[:, :3] += torch.randn((N, 3), generator=g, device="cuda") * 0.6
    model = {"clm_offload": GaussianModelCLMOffload, "no_offload": GaussianModelNoOffload,
             "naive_offload": GaussianModelNaiveOffload}[strategy](3)
    model.create_from_tensors(truth["xyz"] + torch.randn((N, 3), generator=g, device="cuda") * 0.05, noisy_sh,
                              truth["scaling"], truth["rotation"], truth["opacity"], spatial_lr_scale=truth["extent"])
    model.training_setup(args)
    model.split_generator = torch.Generator(device="cuda").manual_seed(5)
    side = {}
    if variant == "exposure":
        side["exposure"] = trainer.build_exposure(cams, IMAGES)
    if variant == "sky":
        side["sky"] = trainer.build_sky(cams, [], IMAGES, shape=(16, 32))

    class Scene:
        cameras_extent = truth["extent"]

    seen = dict(batches=[], evals=[], levels=[])
    real_strategy = trainer._strategy

    def spying_strategy(*a, **k):
        run_batch, render_fn = real_strategy(*a, **k)

        def run(batch):
            out = run_batch(batch)
            seen["batches"].append(dict(sizes={(c.image_width, c.image_height) for c in batch},
                                        images={tuple(c.original_image.shape) for c in batch},
                                        global_size=(utils.get_img_width(), utils.get_img_height()),
                                        peak=torch.cuda.max_memory_allocated()))
            return out

        def render(cam):
            img = render_fn(cam)
            seen["evals"].append((tuple(img.shape), tuple(cam.original_image.shape),
                                  (utils.get_img_width(), utils.get_img_height())))
            return img
        return run, render

    monkeypatch.setattr(trainer, "_strategy", spying_strategy)
    real_levels = trainer.LevelCameras

    def spying_levels(*a, **k):
        lv = real_levels(*a, **k)
        seen["levels"].append(lv)
        return lv

    monkeypatch.setattr(trainer, "LevelCameras", spying_levels)
    log = io.StringIO()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    seen["before"] = torch.cuda.memory_allocated()
    error = None
    try:
        trainer.training(model, Scene, cams, [], log, iterations=IMAGES, test_iterations=(5,), **side)
    except Exception as e:  # noqa: BLE001 -- handed to the test that expects it
        error = e
    torch.cuda.synchronize()
    text = log.getvalue()
    losses = [l.split(" loss: ")[1].split(" image:")[0].split(" depth_l1_weight")[0] for l in text.splitlines() if " loss: " in l]
    params = [t.detach().clone().cpu() for t in (model.get_xyz, model.get_opacity, model.get_scaling, model.get_rotation,
                                                  model.get_features)] if keep_params else None
    return dict(seen, text=text, error=error, losses=losses, params=params, side=side, extra_bytes=extra_bytes,
                size_after=(utils.get_img_width(), utils.get_img_height()), cams=cams)


def _check_schedule(r):
    assert r["error"] is None, r["error"]
    lines = [tuple(int(v) for v in m) for m in LEVEL_LINE.findall(r["text"])]
    assert lines == [(2, 24, 16, 1), (1, 48, 32, 1 + SCHEDULE), (0, 96, 64, 1 + 2 * SCHEDULE)], (lines, r["text"][:600])
    want = [(24, 16)] * 2 + [(48, 32)] * 2 + [(96, 64)] * 4
    assert len(r["batches"]) == IMAGES // BSZ
    for b, (w, h) in zip(r["batches"], want):
        assert b["sizes"] == {(w, h)} and b["images"] == {(3, h, w)} and b["global_size"] == (w, h), (b, w, h)
    # the evaluation at image 5 falls into the coarse phase and reports on full-size images
    assert r["evals"] and all(e == ((3, H, W), (3, H, W), (W, H)) for e in r["evals"]), r["evals"]
    assert "Evaluating train:" in r["text"]
    assert r["size_after"] == (W, H)
    assert len(r["losses"]) == IMAGES // BSZ
    assert all(np.isfinite([float(v) for v in l.split()]).all() for l in r["losses"]), r["losses"]
    assert [lv.level for lv in r["levels"]] == [2, 1]


ENGINES = [("no_offload", "hbm"), ("clm_offload", "hbm"), ("clm_offload", "host"), ("naive_offload", "hbm")]


@pytest.mark.parametrize("strategy,residency", ENGINES, ids=lambda v: v)
def test_trainer_follows_the_schedule(dev, monkeypatch, strategy, residency):
    _check_schedule(_train(monkeypatch, strategy, residency))


@pytest.mark.parametrize("variant", ["exposure", "mask", "sky", "depth"])
def test_trainer_schedule_with_side_models_masks_and_priors(dev, monkeypatch, variant):
    r = _train(monkeypatch, "clm_offload", "hbm", variant=variant)
    _check_schedule(r)
    if variant == "exposure":
        table = r["side"]["exposure"].param.detach().cpu()
        eye = torch.eye(3, 4).expand_as(table)
        assert float((table - eye).abs().max()) > 0, "the rows the views share with their cameras were trained"
    if variant == "sky":
        table = r["side"]["sky"].param.detach().cpu()
        assert float((table - 0.5).abs().max()) > 0, "the one map the views share with their cameras was trained"
    if variant == "mask":
        for lv in r["levels"]:
            for c in r["cams"][:2]:
                v = lv.views[id(c)]
                want, n = R.mask_resample(c.loss_mask.cpu().numpy(), lv.level)
                assert np.array_equal(v.loss_mask.cpu().numpy(), want) and v.loss_mask_count == n
            assert all(lv.views[id(c)].loss_mask is None for c in r["cams"][2:])
    if variant == "depth":
        assert "depth_l1_weight" in r["text"]
        for lv in r["levels"]:
            for c in r["cams"][:2]:
                v = lv.views[id(c)]
                assert np.array_equal(v.invdepth.cpu().numpy(), R.area_resample(c.invdepth.cpu().numpy(), lv.level))


def test_the_global_size_is_restored_after_an_exception(dev, monkeypatch):
    from clm_gs_amd import utils
    r = _train(monkeypatch, "clm_offload", "hbm", break_mask=True)
    assert r["error"] is not None and "mask" in str(r["error"]).lower(), r["error"]
    assert r["size_after"] == (W, H) == (utils.get_img_width(), utils.get_img_height())
    assert r["batches"] == [] or r["batches"][0]["global_size"] == (24, 16)   # it was raised inside the coarse phase


@functools.lru_cache(maxsize=None)
def _off_runs():
    """The same run with untouched default_args() and with the schedule's options spelled out as off."""
    mp = pytest.MonkeyPatch()
    try:
        untouched = _train(mp, "clm_offload", "hbm", num_downscales=0, explicit=False, keep_params=True)
        mp.undo()
        spelled = _train(mp, "clm_offload", "hbm", num_downscales=0, explicit=True, keep_params=True)
    finally:
        mp.undo()
    return untouched, spelled


def test_off_is_the_parent_bit_for_bit(dev):
    untouched, spelled = _off_runs()
    for r in (untouched, spelled):
        assert r["error"] is None and r["levels"] == [] and not LEVEL_LINE.search(r["text"])
        assert all(b["sizes"] == {(W, H)} for b in r["batches"])
    assert untouched["losses"] == spelled["losses"] and len(spelled["losses"]) == IMAGES // BSZ
    for a, b in zip(untouched["params"], spelled["params"]):
        assert torch.equal(a, b)


def test_the_coarse_phase_adds_no_more_than_the_ring(dev, monkeypatch, variant=None):
    """Peak device memory above the pre-training value, up to the last batch of the coarsest level, against the same
    figure of the full-size run: no more than the ring of 2 x bsz level images plus the level's masks and priors (every
    tensor rounded up to the allocator's 512 B, the sizes worked out here)."""
    base = _off_runs()[1]
    r = _train(monkeypatch, "clm_offload", "hbm", variant=variant)
    assert r["error"] is None, r["error"]
    Hs, Ws = R.level_size(H, W, D)
    bound = 2 * BSZ * _alloc(3 * Hs * Ws) + r["extra_bytes"]
    coarse = [b for b in r["batches"] if b["global_size"] == (Ws, Hs)]
    grew = coarse[-1]["peak"] - r["before"]
    base_grew = base["batches"][len(coarse) - 1]["peak"] - base["before"]
    print(f"coarse phase ({variant}): peak - before = {grew} B; full-size run: {base_grew} B; bound on the difference: {bound} B")
    assert grew <= base_grew + bound, (grew, base_grew, bound)
