"""float64 reference of gsplat's absgrad (rasterize_to_pixels(absgrad=True) -> means2d.absgrad; AbsGS), for the tests.

The per-tile dense blend of oracle.gs_oracle.rasterize_to_pixels with the same rules (sigma < 0 skip, 0.999 clamp, 1/255
cut, stop before T <= 1e-4, backgrounds), except that the means enter each tile as a PER-PIXEL leaf [256, K, 2]: autograd
then returns dL_p/dmean2d of every pixel p by itself, and

    absgrad[c, g] = sum_p |dL_p/dmean2d[c, g]|   (componentwise),      plain[c, g] = sum_p dL_p/dmean2d[c, g]

are scattered to the C*N rows.  `plain` is the oracle's autograd v_means2d (tests/test_absgrad_cpu.py holds it to that)."""
import torch


def absgrad_reference(m2, cn, col, op, w, h, off, fids, vi, va=None, bg=None, tile_size=16):
    """m2 [C,N,2], cn [C,N,3], col [C,N,3], op [C,N]; off [C,th,tw], fids [I]: the lists; vi [C,H,W,3] / va [C,H,W]: the
    cotangents of the image and of alpha; bg [C,3] or None.  -> (absgrad [C*N,2], plain [C*N,2]), float64."""
    dt = torch.float64
    C, N = op.shape
    th, tw = off.shape[1:]
    offs = off.flatten().tolist() + [int(fids.shape[0])]
    m2, cn, col, op = m2.reshape(C * N, 2).to(dt), cn.reshape(C * N, 3).to(dt), col.reshape(C * N, 3).to(dt), op.reshape(C * N).to(dt)
    fid = fids.to(torch.int64)
    vi = vi.to(dt)
    va = torch.zeros(C, h, w, dtype=dt) if va is None else va.to(dt)
    out_abs, out_sum = torch.zeros(C * N, 2, dtype=dt), torch.zeros(C * N, 2, dtype=dt)
    ii, jj = torch.meshgrid(torch.arange(tile_size), torch.arange(tile_size), indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    for c in range(C):
        for ty in range(th):
            for tx in range(tw):
                tid = (c * th + ty) * tw + tx
                s, e = offs[tid], offs[tid + 1]
                if e <= s:
                    continue
                K = e - s
                g = fid[s:e]
                y, x = ty * tile_size + ii, tx * tile_size + jj
                inside = (y < h) & (x < w)
                v_rgb, v_al = torch.zeros(256, 3, dtype=dt), torch.zeros(256, dtype=dt)
                v_rgb[inside] = vi[c, y[inside], x[inside]]
                v_al[inside] = va[c, y[inside], x[inside]]
                mp = m2[g][None].expand(256, K, 2).clone().requires_grad_()  # the means, one copy per pixel
                dx = mp[..., 0] - (x.to(dt) + 0.5)[:, None]
                dy = mp[..., 1] - (y.to(dt) + 0.5)[:, None]
                a_, b_, c_ = cn[g, 0][None], cn[g, 1][None], cn[g, 2][None]
                sigma = 0.5 * (a_ * dx * dx + c_ * dy * dy) + b_ * dx * dy
                neg = sigma.detach() < 0
                alpha = torch.clamp(op[g][None] * torch.exp(-torch.where(neg, torch.zeros_like(sigma), sigma)), max=0.999)
                valid = ~neg & (alpha.detach() >= 1.0 / 255.0)
                a_eff = torch.where(valid, alpha, torch.zeros_like(alpha))
                incl = torch.cumprod(1.0 - a_eff, dim=1)
                done = (incl.detach() <= 1e-4) & valid
                anyd = done.any(dim=1)
                first = torch.where(anyd, done.to(torch.int64).argmax(dim=1), torch.full_like(anyd, K, dtype=torch.int64))
                keep = torch.arange(K)[None, :] < first[:, None]
                a_eff = a_eff * keep
                incl = torch.cumprod(1.0 - a_eff, dim=1)
                T_before = torch.cat([torch.ones(256, 1, dtype=dt), incl[:, :-1]], dim=1)
                rgb = (a_eff * T_before) @ col[g]
                T_fin = incl[:, -1]
                if bg is not None:
                    rgb = rgb + T_fin[:, None] * bg[c].to(dt)[None, :]
                loss = (rgb * v_rgb).sum() + ((1.0 - T_fin) * v_al).sum()
                (gp,) = torch.autograd.grad(loss, mp)  # [256, K, 2]: dL_p/dmean2d, pixel by pixel
                out_abs.index_add_(0, g, gp.abs().sum(0))
                out_sum.index_add_(0, g, gp.sum(0))
    return out_abs, out_sum


def case_absgrad(case):
    """absgrad_reference on a raster case of tests/scenes.py."""
    return absgrad_reference(case["m2"], case["cn"], case["col"], case["op"], case["w"], case["h"], case["off"], case["fids"],
                             case["vi"], case["va"], case["bg"])


def oracle_v_means2d(case):
    """The oracle's autograd v_means2d [C*N,2] of sum(img * vi) + sum(alpha * va), float64."""
    from oracle import gs_oracle as O
    a = [case[k].double().requires_grad_() for k in ("m2", "cn", "col", "op")]
    bg = case["bg"].double() if case["bg"] is not None else None
    img, al = O.rasterize_to_pixels(*a, case["w"], case["h"], 16, case["off"], case["fids"], backgrounds=bg)
    ((img * case["vi"].double()).sum() + (al[..., 0] * case["va"].double()).sum()).backward()
    return a[0].grad.reshape(-1, 2)
