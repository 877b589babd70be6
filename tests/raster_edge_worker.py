"""Runs the rasterizer's two tile kernels on the hand-built cases of tests/scenes.py through the C ABI.

As a script (`python -m tests.raster_edge_worker OUTDIR`, the library chosen by CLMGS_LIB_PATH) it runs the fixed inputs
of the special-entry, list-length and non-finite cases and writes every output as OUTDIR/<case>.<output>.npy, so that
tests/test_gpu_raster_edges.py can hold the A/B builds of rasterize.hip to the product library bit for bit.
"""
import math
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import scenes as S  # noqa: E402

GRAD_NAMES = ("means2d", "conics", "colors", "opacities")


def slots_of(fids, n_rows):
    """Emit slots of a list: row r owns the contiguous slots [row_cum[r-1], row_cum[r]), in list order."""
    f = fids.long()
    row_cum = torch.cumsum(torch.bincount(f, minlength=n_rows), 0)
    slot = torch.empty_like(f)
    slot[torch.sort(f, stable=True).indices] = torch.arange(f.numel())
    return slot.to(torch.int32), row_cum


def run(case, dev, atomic=True, slots=True):
    """-> dict: img [C,H,W,3], alpha [C,H,W], last [C,H,W], and the gradients of both backward routes (`atomic_<name>`:
    clmgs_rasterize_bwd with float atomics; `slot_<name>`: emit slots + partial lines + the per-row sum, one camera per
    call as the slot mode takes C == 1), all on the CPU."""
    from clm_gs_amd import _lib
    from clm_gs_amd._lib import check, dptr, stream

    L = _lib.lib()
    C, N = case["op"].shape
    w, h = case["w"], case["h"]
    tw, th = math.ceil(w / 16), math.ceil(h / 16)
    fids_c, off_c = case["fids"], case["off"]
    I = fids_c.numel()
    m2, cn, col, op = (case[k].to(dev).contiguous() for k in ("m2", "cn", "col", "op"))
    bg = case["bg"].to(dev).contiguous() if case["bg"] is not None else None
    off, fids = off_c.to(dev).contiguous(), fids_c.to(dev).contiguous()
    vi, va = case["vi"].to(dev).contiguous(), case["va"].to(dev).contiguous()
    out = torch.full((C, h, w, 3), float("nan"), device=dev)
    al = torch.full((C, h, w), float("nan"), device=dev)
    last = torch.full((C, h, w), -7, dtype=torch.int32, device=dev)
    packed = torch.empty(C * N, 16, device=dev)
    check(L.clmgs_rasterize_fwd(stream(), C, N, I, dptr(m2), dptr(cn), dptr(col), dptr(op), dptr(bg, None, True), w, h, 16,
                                tw, th, dptr(off), dptr(fids), dptr(packed), dptr(out), dptr(al), dptr(last)))
    res = {"img": out, "alpha": al, "last": last}

    def grads(Cn):
        return [torch.full((Cn, N, 2), float("nan"), device=dev), torch.full((Cn, N, 3), float("nan"), device=dev),
                torch.full((Cn, N, 3), float("nan"), device=dev), torch.full((Cn, N), float("nan"), device=dev)]

    if atomic:
        pg = torch.full((C * N, 16), float("nan"), device=dev)
        outs = grads(C)
        check(L.clmgs_rasterize_bwd(stream(), C, N, I, dptr(packed), dptr(bg, None, True), w, h, 16, tw, th, dptr(off),
                                    dptr(fids), dptr(al), dptr(last), dptr(vi), dptr(va), dptr(pg),
                                    *[dptr(x) for x in outs], None, None, None))
        res.update({f"atomic_{n}": x for n, x in zip(GRAD_NAMES, outs)})
    if slots:
        per_cam = []
        bounds = off_c.reshape(C, -1)[:, 0].tolist() + [I]
        LF = L.clmgs_rasterize_partials_bytes(1) // 4
        for c in range(C):
            s0, e0 = bounds[c], bounds[c + 1]
            f = fids_c[s0:e0] - c * N  # this camera's list with row ids and list indices of its own
            slot, row_cum = slots_of(f, N)
            fd, sd, rd = f.to(dev).contiguous(), slot.to(dev), row_cum.to(dev)
            oc = (off[c:c + 1] - s0).contiguous()
            lc = (last[c:c + 1] - s0).contiguous()
            parts = torch.full((max(e0 - s0, 1), LF), float("nan"), device=dev)  # every line must be written
            pg = torch.full((N, 16), float("nan"), device=dev)
            outs = grads(1)
            check(L.clmgs_rasterize_bwd(stream(), 1, N, e0 - s0, dptr(packed[c * N:(c + 1) * N]),
                                        dptr(bg[c:c + 1] if bg is not None else None, None, True), w, h, 16, tw, th,
                                        dptr(oc), dptr(fd), dptr(al[c:c + 1]), dptr(lc), dptr(vi[c:c + 1].contiguous()),
                                        dptr(va[c:c + 1].contiguous()), dptr(pg), *[dptr(x) for x in outs],
                                        dptr(sd), dptr(rd), dptr(parts)))
            per_cam.append(outs)
        res.update({f"slot_{n}": torch.cat([p[i] for p in per_cam]) for i, n in enumerate(GRAD_NAMES)})
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in res.items()}


def fixed_cases():
    """name -> case: the inputs the A/B builds are compared on (special entries, list lengths, non-finite rows)."""
    cases = {"special": S.special_entry_case()}
    for K in S.LIST_LENGTHS:
        for sat in (False, True):
            for layout in ("single", "middle"):
                cases[f"list{K}_{'sat' if sat else 'tr'}_{layout}"] = S.list_case(K, sat, layout)
    bad, zero, _ = S.nonfinite_case()
    cases["nonfinite"], cases["nonfinite_zero"] = bad, zero
    return cases


def main(outdir):
    dev = torch.device("cuda:0")
    for name, case in fixed_cases().items():
        for k, v in run(case, dev).items():
            np.save(os.path.join(outdir, f"{name}.{k}.npy"), v.numpy())
    print("raster_edge_worker ok:", os.environ.get("CLMGS_LIB_PATH", "default library"))


if __name__ == "__main__":
    main(sys.argv[1])
