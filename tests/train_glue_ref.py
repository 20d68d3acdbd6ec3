"""Plain float64 numpy references of the training step's view branch and row glue (csrc/k_train_head.hip, k_train_rows.hip,
k_small_matmul of k_step_io.hip), written from the formulas in the kernels' header comments and include/danbo_hip.h, the inputs
of every case tests/test_gpu_train_glue.py runs, and the error bound of every output.  tests/test_train_glue_host.py proves the
references against torch.autograd and the bounds against deliberately wrong references, without a GPU.

Every function that sums returns, next to the sum, the sum of the absolute values of its terms per output entry: a result
formed by n fp32 roundings over the terms t_i lies within  n 2^-24 sum |t_i| (1 + 1e-3)  of the float64 value (`bound`)."""
import zlib

import numpy as np

F64, F32 = np.float64, np.float32
U = 2.0 ** -24                    # unit round-off of fp32
HW, HVW, J = 256, 128, 24         # trunk width, view-layer width, bones
CU = 256                          # compute units of a full MI355X (the GPU tests ask danbo_device_info)
VG_SLICES = 32                    # ray slices of k_train_view_grad


def bound(n, abs_sum):
    return n * U * np.asarray(abs_sum, F64) * (1 + 1e-3)


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f64(x):
    return np.asarray(x, F64)


# ----------------------------------------------------------------------------- the references
def view_inputs(rays_d, L, ldv, skts=None, G=1, normalise=False, codes=None, cam_idx=None):
    """-> vin [R, ldv] = [d | sin(2^l d), cos(2^l d) for l < L | code of the clamped camera | 0], and d [R, 3]"""
    d = f64(rays_d)
    R = d.shape[0]
    if skts is not None:          # root-local rays: skts[g, 0, :3, :3] d, pose g owning R / G consecutive rays
        rot = f64(skts)[np.arange(R) // (R // G), 0, :3, :3]
        d = np.einsum("rij,rj->ri", rot, d)
    if normalise:
        d = d / np.maximum(np.sqrt((d * d).sum(-1, keepdims=True)), 1e-12)
    cols = [d]
    for l in range(L):
        cols += [np.sin(2.0 ** l * d), np.cos(2.0 ** l * d)]
    cols = np.concatenate(cols, 1)
    out = np.zeros((R, ldv), F64)
    out[:, :cols.shape[1]] = cols
    if codes is not None:
        cam = np.zeros(R, np.int64) if cam_idx is None else np.clip(np.asarray(cam_idx, np.int64), 0, len(codes) - 1)
        out[:, cols.shape[1]:cols.shape[1] + codes.shape[1]] = f64(codes)[cam]
    return out, d


def cview(vin, views_w, b_eff, view_ch):
    """cview[r] = W_v[:, 256:] vin[r, :view_ch] + b_eff -> [R, 128], sum |terms|"""
    v, w = f64(vin)[:, :view_ch], f64(views_w)[:, HW:HW + view_ch]
    return f64(b_eff)[None] + v @ w.T, np.abs(f64(b_eff))[None] + np.abs(v) @ np.abs(w).T


def ray_grad(dpre_v, row_ray, R):
    """d cview[ray] = sum of d pre_v over the ray's rows (row_ray clamped to [0, R)) -> [R, 128], sum |terms|, rows per ray"""
    ray = np.clip(np.asarray(row_ray, np.int64), 0, R - 1)
    out, ab = np.zeros((R, HVW), F64), np.zeros((R, HVW), F64)
    np.add.at(out, ray, f64(dpre_v))
    np.add.at(ab, ray, np.abs(f64(dpre_v)))
    return out, ab, np.bincount(ray, minlength=R)


def view_grad(d_cview, vin, view_ch, cam_idx=None, n_codes=0):
    """d W_v[:, 256:] = d cview^T vin [128, view_ch]; csum[cam] = sum of d cview over the rays of the (clamped) camera
    -> (gw, sum |terms|), (csum, sum |terms|, rays per camera) or None"""
    dc, v = f64(d_cview), f64(vin)[:, :view_ch]
    gw = (dc.T @ v, np.abs(dc).T @ np.abs(v))
    if n_codes == 0:
        return gw, None
    R = dc.shape[0]
    cam = np.zeros(R, np.int64) if cam_idx is None else np.clip(np.asarray(cam_idx, np.int64), 0, n_codes - 1)
    cs, ab = np.zeros((n_codes, HVW), F64), np.zeros((n_codes, HVW), F64)
    np.add.at(cs, cam, dc)
    np.add.at(ab, cam, np.abs(dc))
    return gw, (cs, ab, np.bincount(cam, minlength=n_codes))


def head_chain(g_wfv, g_beff, csum, feature_w, feature_b, views_w, n_codes=0, code_size=0, code_col0=0):
    """The merged layer's gradient pulled back to feature_linear and views_linears.0 (W_fv = W_v[:, :256] W_f,
    b_eff = b_v + W_v[:, :256] b_f) -> {name: (value, sum |terms|)} for g_views_w_a (= d W_v[:, :256]), g_feature_w, g_feature_b,
    g_views_b and, with frame codes, g_codes"""
    gw, gb, wf, bf, wv = f64(g_wfv), f64(g_beff), f64(feature_w), f64(feature_b), f64(views_w)
    wa = wv[:, :HW]
    out = dict(g_views_w_a=(gw @ wf.T + np.outer(gb, bf), np.abs(gw) @ np.abs(wf).T + np.abs(np.outer(gb, bf))),
               g_feature_w=(wa.T @ gw, np.abs(wa).T @ np.abs(gw)),
               g_feature_b=(wa.T @ gb, np.abs(wa).T @ np.abs(gb)),
               g_views_b=(gb, np.abs(gb)))
    if n_codes:
        wc = wv[:, HW + code_col0:HW + code_col0 + code_size]
        out["g_codes"] = (f64(csum) @ wc, np.abs(f64(csum)) @ np.abs(wc))
    return out


def loss_grad(rgb, acc, rgb0, acc0, target, bgs, use_bg, mse, w_fine, w_coarse):
    """trainer.py's L1 / MSE on rgb + (1 - acc) bg, mean over R x 3, for the fine and the coarse pass.  bgs None: background 1.
    -> {g_rgb, g_acc, g_rgb0, g_acc0: (value, sum |terms|)}, loss (2,) and its sum |terms| (2,)"""
    R = len(acc)
    t = f64(target)
    bg = (np.ones((R, 3)) if bgs is None else f64(bgs)) if use_bg else np.zeros((R, 3))
    inv = 1.0 / (3.0 * R)
    out, loss = {}, np.zeros(2)
    for p, (c, a, w) in enumerate(((rgb, acc, w_fine), (rgb0, acc0, w_coarse))):
        c, a, w = f64(c), f64(a)[:, None], float(F32(w))
        e = c + (1.0 - a) * bg - t
        mag = np.abs(c) + np.abs((1.0 - a) * bg) + np.abs(t)         # the terms of e
        g = (2.0 * e if mse else np.sign(e)) * inv * w
        g_abs = (2.0 * mag if mse else np.abs(np.sign(e))) * inv * w
        sfx = "0" if p else ""
        out["g_rgb" + sfx] = (g, g_abs)
        out["g_acc" + sfx] = (-(g * bg).sum(-1), (g_abs * np.abs(bg)).sum(-1))
        loss[p] = ((e * e if mse else np.abs(e)) * inv * w).sum()
    return out, loss, loss.copy()                                      # every term of a loss sum is >= 0


def draw_unmerge(d_raw_c, d_raw_sorted, order, bits_c, bits_f, weights, alpha):
    """Un-merge of the final composite's d raw (sorted order) onto the coarse (+ the coarse composite's own gradient: ONE fp32
    addition per component, stated here as that addition) and the importance samples; labels (weights alpha > 0) in un-sorted
    order; the sum of the samples outside every volume per ray; the number of labels outside.
    -> dict: d_raw_c, d_raw_f (fp32, exact), label_c, label_f (uint8), d_raw_rows (value, sum |terms|), n_outside, maxabs_inside"""
    d_raw_c, ds = np.asarray(d_raw_c, F32), np.asarray(d_raw_sorted, F32)
    R, S = d_raw_c.shape[:2]
    St = ds.shape[1]
    Sf = St - S
    comb, df = d_raw_c.copy(), np.zeros((R, Sf, 4), F32)
    lab = (f64(weights) * f64(alpha) > 0).astype(np.uint8)
    lc, lf = np.zeros((R, S), np.uint8), np.zeros((R, Sf), np.uint8)
    order = np.asarray(order, np.int64)
    rr = np.arange(R)[:, None].repeat(St, 1)
    is_c = order < S
    comb[rr[is_c], order[is_c]] = ds[is_c] + d_raw_c[rr[is_c], order[is_c]]          # float32 + float32
    lc[rr[is_c], order[is_c]] = lab[is_c]
    df[rr[~is_c], order[~is_c] - S] = ds[~is_c]
    lf[rr[~is_c], order[~is_c] - S] = lab[~is_c]
    out_c, out_f = np.asarray(bits_c) == 0, np.asarray(bits_f) == 0
    rows = (f64(comb) * out_c[..., None]).sum(1) + (f64(df) * out_f[..., None]).sum(1)
    rows_abs = (np.abs(f64(comb)) * out_c[..., None]).sum(1) + (np.abs(f64(df)) * out_f[..., None]).sum(1)
    inside = np.concatenate([np.abs(comb[~out_c]).ravel(), np.abs(df[~out_f]).ravel(), np.zeros(1, F32)]).max()
    return dict(d_raw_c=comb, d_raw_f=df, label_c=lc, label_f=lf, d_raw_rows=(rows, rows_abs),
                n_outside=int(lc[out_c].sum()) + int(lf[out_f].sum()), maxabs_inside=F32(inside))


def bone_lists(bits_c, bits_f, row_sample, R, n_c, n_f):
    """rows R .. R + n_c + n_f of a step: row i is sample row_sample[i] of the coarse pass (i < R + n_c) or of the importance pass;
    bone j's list holds the rows whose sample has bit j set -> [set of rows] * 24, cntb [24]"""
    bc, bf = np.asarray(bits_c).ravel(), np.asarray(bits_f).ravel()
    sets = [set() for _ in range(J)]
    for i in range(R, R + n_c + n_f):
        b = int(bc[row_sample[i]] if i < R + n_c else bf[row_sample[i]])
        for j in range(J):
            if (b >> j) & 1:
                sets[j].add(i)
    return sets, np.array([len(s) for s in sets], np.int32)


def small_matmul(A, B, bias=None):
    """A [M,K] @ B [K,N] + bias[N] -> value, sum |terms|"""
    a, b = f64(A), f64(B)
    z = np.zeros(b.shape[1]) if bias is None else f64(bias)
    return a @ b + z[None], np.abs(a) @ np.abs(b) + np.abs(z)[None]


# ----------------------------------------------------------------------------- cases and inputs (shared by the host and GPU tests)
def round4(n):
    return (n + 3) // 4 * 4


# view_inputs: (ray_mode, G) and the rays of a case; R % G == 0 is the entry point's contract, so G = 3 runs 3 and 39 rays
VI_L = (0, 4)
VI_MODES = ((0, 1), (1, 1), (1, 3))
VI_CODES = ("none", "cam_null", "in_range", "out_of_range")
VI_CF, VI_NCODES = 16, 4


def vi_rays(G):
    return (1, 37) if G == 1 else (G, 13 * G)


def rotations(rng, n):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q


def view_inputs_case(L, ray_mode, G, normalise, code_mode, ldv_extra, R):
    rng = rng_of("vi", L, ray_mode, G, normalise, code_mode, ldv_extra, R)
    d = rng.normal(size=(R, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.3, 1.0, size=(R, 1))).astype(F32)       # |d| <= 1
    skts = None
    if ray_mode == 1:
        skts = rng.normal(size=(G, J, 4, 4)).astype(F32)
        skts[:, :, :3, :3] = rotations(rng, G * J).reshape(G, J, 3, 3) * 0.999
    codes = cam = None
    if code_mode != "none":
        codes = rng.normal(size=(VI_NCODES, VI_CF)).astype(F32)
        if code_mode == "in_range":
            cam = rng.integers(0, VI_NCODES, size=R)
        elif code_mode == "out_of_range":
            cam = rng.integers(0, VI_NCODES, size=R)
            cam[::2] = -1
            cam[1::2] = VI_NCODES + 5
            cam[R // 2] = 2 if R > 2 else cam[R // 2]
    nd = 3 * (1 + 2 * L)
    ldv = round4(nd + (VI_CF if codes is not None else 0)) + ldv_extra
    return dict(rays_d=d, skts=skts, G=G, ray_mode=ray_mode, normalise=normalise, L=L, codes=codes, cam_idx=cam, ldv=ldv, R=R, nd=nd)


def view_inputs_expect(c):
    """-> vin64 [R, ldv], bound [R, ldv]: 3 2^-24 |d| on the direction columns (rotation, norm and division round the vector
    about three times), 2e-7 (pe_sincos' stated accuracy) + 2^L 3 2^-24 (that argument error scaled by 2^l) on the sin / cos
    columns, 0 (bit-exact) on the frame code and the zero pad"""
    ref, d = view_inputs(c["rays_d"], c["L"], c["ldv"], c["skts"], c["G"], bool(c["normalise"]), c["codes"], c["cam_idx"])
    b = np.zeros_like(ref)
    b[:, :3] = 3 * U * np.linalg.norm(d, axis=-1, keepdims=True)
    b[:, 3:c["nd"]] = 2e-7 + 2.0 ** c["L"] * 3 * U
    return ref, b


CVIEW_CH = (0, 3, 27, 64, 160)


def cview_rays(cu=CU):
    return (1, 7, 8, 9, 8 * 8 * cu + 13)


def view_weights(rng, view_ch):
    """views_linears.0.weight [128, 256 + view_ch] at the initialiser's scale"""
    return (rng.normal(size=(HVW, HW + view_ch)) / np.sqrt(HW + view_ch)).astype(F32)


def cview_case(view_ch, R):
    rng = rng_of("cview", view_ch, R)
    ldv = round4(view_ch) + 4                                  # ldv > view_ch: the columns behind view_ch are never read (NaN)
    vin = np.full((R, ldv), np.nan, F32)
    vin[:, :view_ch] = rng.uniform(-1, 1, size=(R, view_ch))
    return dict(vin=vin, ldv=ldv, view_ch=view_ch, R=R, views_w=view_weights(rng, view_ch), b_eff=rng.normal(0.3, 0.2, size=HVW).astype(F32))


def cview_expect(c):
    ref, ab = cview(c["vin"], c["views_w"], c["b_eff"], c["view_ch"])
    return ref, bound(c["view_ch"] + 1, ab)                    # n = view_ch + 1: the bias start value and one fma per column


VG_ROWS = (1, 15, 16, 17, 63, 64, 65, 129, 1000)
VG_R = (1, 5, 31, 32, 33, 256, 261)
VG_CH = (27, 64)
VG_PATTERNS = ("one_per_row", "long_runs", "split_runs", "clamped")
VG_CAMS = ("no_codes", "sorted", "interleaved", "cam_null", "out_of_range")
VG_NCODES = 4


def vg_big_rows(cu=CU):
    return 64 * 8 * cu + 1                                     # one row more than one sweep of k_train_ray_grad's grid covers


def row_ray_pattern(rng, pattern, rows, R):
    i = np.arange(rows)
    if pattern == "one_per_row":
        return (i % R).astype(np.int32)
    if pattern == "long_runs":                                 # runs of 11 and 75 rows: they cross the 8-row batches and the 64-row chunks
        return ((i // 11 + i // 75) % R).astype(np.int32)
    if pattern == "split_runs":                                # ray 0 owns every third run of 5 rows, random rays in between
        other = rng.integers(0, R, size=rows // 5 + 1)
        return np.where((i // 5) % 3 == 0, 0, other[i // 5]).astype(np.int32)
    assert pattern == "clamped"
    ray = ((i // 3) % R).astype(np.int32)
    ray[::7] = -3
    ray[3::7] = R + 2
    return ray


def view_grads_case(rows, R, view_ch, pattern, cam_mode, cheap=False):
    """d pre_v of `rows` rows (row order; the tests put it into fragment order), row_ray, vin, cam_idx.  The values lean positive
    (mean 1) so that no sum cancels to nothing beside its terms."""
    rng = rng_of("vg", rows, R, view_ch, pattern, cam_mode)
    if cheap:
        dpre = (1.0 + ((np.arange(rows)[:, None] * 7 + np.arange(HVW)[None] * 3) % 64) / 64.0).astype(F32)
    else:
        dpre = rng.normal(1.0, 0.5, size=(rows, HVW)).astype(F32)
    ldv = round4(view_ch) + 4
    vin = np.full((R, ldv), np.nan, F32)
    vin[:, :view_ch] = rng.normal(0.5, 0.5, size=(R, view_ch))
    cam, n_codes = None, VG_NCODES
    if cam_mode == "no_codes":
        n_codes = 0
    elif cam_mode == "sorted":
        cam = np.sort(rng.integers(0, n_codes, size=R))
    elif cam_mode == "interleaved":
        cam = (np.arange(R) % n_codes)
    elif cam_mode == "out_of_range":
        cam = rng.integers(-2, n_codes + 3, size=R)
    else:
        assert cam_mode == "cam_null"
    return dict(rows=rows, R=R, view_ch=view_ch, dpre=dpre, row_ray=row_ray_pattern(rng, pattern, rows, R), vin=vin, ldv=ldv,
                cam_idx=None if cam is None else cam.astype(np.int64), n_codes=n_codes,
                g_prefill=rng.normal(size=(HVW, HW + view_ch)).astype(F32))


def vg_cases_by_rows(rows):
    """(rows, R, view_ch, pattern, cam_mode) of one `rows`: every row_ray pattern and view_ch, R and the cameras cycled"""
    i = VG_ROWS.index(rows)
    return [(rows, VG_R[(i + j) % len(VG_R)], ch, pattern, VG_CAMS[(i + j + k) % len(VG_CAMS)])
            for j, pattern in enumerate(VG_PATTERNS) for k, ch in enumerate(VG_CH)]


def vg_cases_by_rays(R):
    """(rows, R, view_ch, pattern, cam_mode) of one R: every camera mode and view_ch, rows 129 / 1000 and the patterns cycled"""
    i = VG_R.index(R)
    return [((129, 1000)[(i + j) % 2], R, ch, VG_PATTERNS[(i + j + k) % len(VG_PATTERNS)], cam)
            for j, cam in enumerate(VG_CAMS) for k, ch in enumerate(VG_CH)]


def vg_case_big(cu=CU):
    return view_grads_case(vg_big_rows(cu), 261, 64, "long_runs", "sorted", cheap=True)


def ray_grad_expect(c):
    ref, ab, n = ray_grad(c["dpre"], c["row_ray"], c["R"])
    return ref, bound(np.maximum(n, 1)[:, None], ab)           # n = the ray's rows: one addition each, in any order


def view_grad_expect(c, d_cview, prefill=None):
    """from the d cview handed in (the GPU test: the kernel's own) -> gw [128, view_ch] (+ prefill), its bound, csum, its bound"""
    (gw, gw_abs), cs = view_grad(d_cview, c["vin"], c["view_ch"], c["cam_idx"], c["n_codes"])
    if prefill is not None:
        gw, gw_abs = gw + f64(prefill), gw_abs + np.abs(f64(prefill))
    out = [gw, bound(c["R"] + VG_SLICES, gw_abs)]              # n = R + 32: one fma per ray, one addition per ray slice (+ the prefill's)
    if cs is None:
        return out + [None, None]
    return out + [cs[0], bound(np.maximum(cs[2], 1)[:, None], cs[1])]      # n = the camera's rays


HC_CASES = ((27, 0, 0), (27, 4, 0), (64, 0, 4), (64, 4, 4))    # (view_ch, n_codes, L_view): code_col0 = 3 (1 + 2 L)
HC_CODE = 16


def head_chain_case(view_ch, n_codes, L):
    rng = rng_of("hc", view_ch, n_codes, L)
    n = lambda *s: rng.normal(size=s).astype(F32)      # noqa: E731
    return dict(view_ch=view_ch, n_codes=n_codes, code_size=HC_CODE, code_col0=3 * (1 + 2 * L), g_wfv=n(HVW, HW), g_beff=n(HVW),
                csum=n(max(n_codes, 1), HVW), feature_w=(n(HW, HW) / 16).astype(F32), feature_b=n(HW), views_w=view_weights(rng, view_ch),
                g_prefill=n(HVW, HW + view_ch))


def head_chain_expect(c):
    """-> {name: (ref, bound)}; n: 257 for d W_v[:, :256] (the start value's product, 256 fmas), 128 for the sums over the view
    layer's 128 rows, 0 for the copied bias gradient"""
    e = head_chain(c["g_wfv"], c["g_beff"], c["csum"], c["feature_w"], c["feature_b"], c["views_w"], c["n_codes"], c["code_size"], c["code_col0"])
    n = dict(g_views_w_a=257, g_feature_w=128, g_feature_b=128, g_views_b=0, g_codes=128)
    return {k: (v[0], bound(n[k], v[1])) for k, v in e.items()}


def loss_rays(cu=CU):
    return (1, 255, 256, 257, 2 * 256 * cu + 37)


LOSS_BG = ("no_bg", "bgs", "bgs_null")


def loss_case(R, mse, bg_mode):
    """rgb / rgb0 are built in float64 from the target so that every |e| >= 1e-3 before rounding to fp32 (>= 1e-4 after), except
    a block with use_bg = 0 whose fine rgb equals the target exactly: the L1 sign is never ill-conditioned"""
    rng = rng_of("loss", R, mse, bg_mode)
    target, bgs = rng.uniform(size=(R, 3)).astype(F32), rng.uniform(size=(R, 3)).astype(F32)
    acc, acc0 = (rng.uniform(size=R) * 1.2).astype(F32), (rng.uniform(size=R) * 1.2).astype(F32)      # acc > 1 on some rays
    use_bg = int(bg_mode != "no_bg")
    bg = np.zeros((R, 3)) if not use_bg else (np.ones((R, 3)) if bg_mode == "bgs_null" else f64(bgs))
    delta = lambda: rng.uniform(1e-3, 0.5, size=(R, 3)) * rng.choice([-1.0, 1.0], size=(R, 3))      # noqa: E731
    rgb = (f64(target) - (1.0 - f64(acc)[:, None]) * bg + delta()).astype(F32)
    rgb0 = (f64(target) - (1.0 - f64(acc0)[:, None]) * bg + delta()).astype(F32)
    if not use_bg and R > 5:
        rgb[:5] = target[:5]
    c = dict(rgb=rgb, acc=acc, rgb0=rgb0, acc0=acc0, target=target, bgs=bgs if bg_mode == "bgs" else None, use_bg=use_bg, mse=mse, R=R,
             w_fine=1.0, w_coarse=0.3)
    for col, a in ((rgb, acc), (rgb0, acc0)):
        e = np.abs(f64(col) + (1.0 - f64(a)[:, None]) * bg - f64(target))
        assert ((e >= 1e-4) | (e == 0)).all() and (use_bg == 0 or (e > 0).all())
    return c


def loss_expect(c):
    """-> {name: (ref, bound)} with n = 4 for the gradients, and (loss, bound) with n = 3 R + 8"""
    out, loss, loss_abs = loss_grad(c["rgb"], c["acc"], c["rgb0"], c["acc0"], c["target"], c["bgs"], c["use_bg"], c["mse"], c["w_fine"], c["w_coarse"])
    return {k: (v[0], bound(4, v[1])) for k, v in out.items()}, (loss, bound(3 * c["R"] + 8, loss_abs))


DU_SHAPES = ((5, 3), (48, 16), (130, 64), (200, 56))
DU_BITS = ("all_inside", "all_outside", "mixed")


def du_rays(cu=CU):
    return (1, 157, 2 * 4 * cu + 37)


def draw_unmerge_case(S, Sf, R, bits_mode):
    rng = rng_of("du", S, Sf, R, bits_mode)
    St = S + Sf
    n = lambda *s: rng.normal(size=s).astype(F32)      # noqa: E731

    def bits(*s):
        b = rng.integers(1, 1 << J, size=s).astype(np.uint32)
        if bits_mode == "all_outside":
            b[:] = 0
        elif bits_mode == "mixed":
            b[rng.uniform(size=s) < 0.5] = 0
        return b

    def zero_or_big(*s):            # exactly 0, or >= 1e-10: the fp32 product of two of them is 0 or a normal number
        v = np.exp(rng.uniform(np.log(1e-10), 0.0, size=s))
        v[rng.uniform(size=s) < 0.3] = 0.0
        return v.astype(F32)
    order = np.argsort(rng.uniform(size=(R, St)), axis=1).astype(np.int32)
    return dict(R=R, S=S, Sf=Sf, d_raw_c=n(R, S, 4), d_raw_sorted=n(R, St, 4), order=order, bits_c=bits(R, S), bits_f=bits(R, Sf),
                weights=zero_or_big(R, St), alpha=zero_or_big(R, St))


def draw_unmerge_expect(c):
    e = draw_unmerge(c["d_raw_c"], c["d_raw_sorted"], c["order"], c["bits_c"], c["bits_f"], c["weights"], c["alpha"])
    e["d_raw_rows"] = (e["d_raw_rows"][0], bound(c["S"] + c["Sf"], e["d_raw_rows"][1]))         # n = S + Sf additions at most
    return e


BL_ROWS = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
BL_FIRST = ("start", "middle", "end")
BL_BITS = ("bone0", "bone23", "all24", "none", "random")


def bone_lists_case(rows, first, bits_mode):
    rng = rng_of("bl", rows, first, bits_mode)
    R, n_samples = 11, 333
    mid = rows // 2 if (rows // 2) % 64 else max(rows // 2 - 27, 0)          # first_f off every wavefront boundary
    n_c = {"start": 0, "middle": mid, "end": rows}[first]

    def bits():
        if bits_mode == "random":
            return (rng.integers(0, 1 << J, size=n_samples) * (rng.uniform(size=n_samples) < 0.7)).astype(np.uint32)
        return np.full(n_samples, {"bone0": 1, "bone23": 1 << 23, "all24": (1 << J) - 1, "none": 0}[bits_mode], np.uint32)
    return dict(R=R, rows=rows, n_c=n_c, n_f=rows - n_c, bits_c=bits(), bits_f=bits(),
                row_sample=rng.integers(0, n_samples, size=R + rows + 5).astype(np.int32))


SM_SHAPES = ((1, 1, 1), (3, 130, 195), (128, 16, 256))


def small_matmul_case(M, N, K, with_bias):
    rng = rng_of("sm", M, N, K, with_bias)
    return dict(A=rng.normal(0.3, 1.0, size=(M, K)).astype(F32), B=rng.normal(0.3, 1.0, size=(K, N)).astype(F32),
                bias=rng.normal(size=N).astype(F32) if with_bias else None)


def small_matmul_expect(c):
    """float64 accumulation rounded once: 2^-24 |ref| for the rounding, K 2^-53 sum |terms| for the float64 sum"""
    ref, ab = small_matmul(c["A"], c["B"], c["bias"])
    return ref, (U * np.abs(ref) + c["A"].shape[1] * 2.0 ** -53 * ab) * (1 + 1e-3)
