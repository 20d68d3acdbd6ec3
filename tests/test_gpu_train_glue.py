"""The small hand-written kernels between the large stages of the fused training step (csrc/k_train_head.hip, k_train_rows.hip,
k_small_matmul), each called through its C entry point and held against the float64 references of tests/train_glue_ref.py.

Every output buffer is filled with a sentinel before the call, so that exactly the documented entries are written; every
readable-but-unused input region (fragment-order padding rows, vin columns behind view_ch) holds NaN; and every error bound is
derived: a result formed by n fp32 roundings over the terms t_i lies within n 2^-24 sum |t_i| (1 + 1e-3) of the float64 value,
with n stated at each check (train_glue_ref.*_expect).  Each test prints its worst error / bound ratio."""
import ctypes

import numpy as np
import pytest
import torch

import train_glue_ref as ref
from helpers import DEV, EINVAL

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SENT = -777.25                      # sentinel of the float outputs: no result of these inputs


@pytest.fixture(scope="module")
def lib():
    from core import _hip
    return _hip.lib()


@pytest.fixture(scope="module")
def cu(lib):
    n = ctypes.c_int(0)
    assert lib.danbo_device_info(ctypes.byref(n), None, None, 0) == 0 and n.value > 0
    return n.value


def dev(x):
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(DEV)          # (bit masks travel as int32)


def sent(*shape, value=SENT, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(lib, name, *args):
    """one entry point on the current stream, waited for.  numpy arguments are uploaded and, like every tensor, stay referenced
    until the launch has finished (a temporary freed earlier would hand its memory to the next upload)"""
    from core import _hip
    held = [dev(a) if isinstance(a, np.ndarray) else a for a in args]
    _hip.check(getattr(lib, name)(*(P(a) if isinstance(a, torch.Tensor) else a for a in held), stream()), name)
    torch.cuda.synchronize()


def host(t):
    return t.detach().cpu().numpy()


class Worst:
    """the worst error / bound ratio of a test's checks, printed once at its end"""

    def __init__(self, name):
        self.name, self.ratio, self.checks = name, 0.0, 0

    def check(self, what, got, want, bnd):
        got, want = np.asarray(got, F64), np.asarray(want, F64)
        bnd = np.broadcast_to(np.asarray(bnd, F64), want.shape)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert np.isfinite(got).all(), (what, "not finite")
        err = np.abs(got - want)
        above = int((err > bnd).sum())
        ratio = float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))
        if above:
            i = np.unravel_index(np.argmax(err - bnd), err.shape)
            print(f"{self.name} {what}: {above} entries above their bound, worst at {i}: got {got[i]!r} want {want[i]!r} bound {bnd[i]:.3e}")
        self.ratio, self.checks = max(self.ratio, ratio), self.checks + 1
        assert above == 0, (what, above, ratio)                  # entries above their bound: 0 (a bound of 0 is bit-exactness)

    def done(self):
        print(f"{self.name}: worst error / bound = {self.ratio:.3f} over {self.checks} checks")
        assert self.checks > 0 and self.ratio <= 1.0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- danbo_train_view_inputs
@pytest.mark.parametrize("normalise", [0, 1])
@pytest.mark.parametrize("ray_mode,G", ref.VI_MODES)
@pytest.mark.parametrize("L_view", ref.VI_L)
def test_view_inputs(lib, L_view, ray_mode, G, normalise):
    w = Worst(f"view_inputs L={L_view} mode={ray_mode} G={G} normalise={normalise}")
    for code_mode in ref.VI_CODES:                 # codes = NULL; cam_idx = NULL; in range; -1 and n_codes + 5 (clamped)
        for ldv_extra in (0, 8):                   # ldv = the content width rounded up to 4, and 8 more
            for R in ref.vi_rays(G):               # 1 and 37 rays (3 and 39 for three poses: R % G == 0)
                c = ref.view_inputs_case(L_view, ray_mode, G, normalise, code_mode, ldv_extra, R)
                vin = sent(R + 1, c["ldv"])
                codes, cam = dev(c["codes"]), dev(c["cam_idx"])
                call(lib, "danbo_train_view_inputs", c["rays_d"], c["skts"], R, G, ray_mode, normalise, L_view, codes,
                     ref.VI_NCODES if codes is not None else 0, ref.VI_CF, cam, vin, c["ldv"])
                got = host(vin)
                assert (got[R] == SENT).all()                                       # nothing behind the last ray
                want, bnd = ref.view_inputs_expect(c)
                # direction: 3 2^-24 |d|; sin / cos: 2e-7 + 2^L 3 2^-24; frame code and the zero pad: bit-exact (bound 0)
                w.check((code_mode, ldv_extra, R), got[:R], want, bnd)
                width = c["nd"] + (ref.VI_CF if codes is not None else 0)
                assert not got[:R, width:].any() and c["ldv"] - width >= ldv_extra  # the pad columns are WRITTEN, as 0
                if not ray_mode and not normalise:
                    assert same(got[:R, :3], c["rays_d"])
    w.done()


# ----------------------------------------------------------------------------- danbo_train_cview
@pytest.mark.parametrize("view_ch", ref.CVIEW_CH)
def test_cview(lib, cu, view_ch):
    w = Worst(f"cview view_ch={view_ch}")
    for R in ref.cview_rays(cu):                   # 1, 7, 8, 9: around the 8 rays of a workgroup; 8 * 8 * cu + 13: the grid-stride loop iterates
        c = ref.cview_case(view_ch, R)             # ldv > view_ch, NaN behind view_ch
        out = sent(R + 3, 128)
        call(lib, "danbo_train_cview", c["vin"], c["ldv"], view_ch, c["views_w"], c["b_eff"], R, out)
        got = host(out)
        assert (got[R:] == SENT).all()                                              # rows >= R are left alone
        want, bnd = ref.cview_expect(c)
        w.check(R, got[:R], want, bnd)                                              # n = view_ch + 1
    w.done()


def test_cview_refuses_more_view_inputs_than_its_lds_rows_hold(lib):
    c = ref.cview_case(160, 3)
    out = sent(3, 128)
    vin, views_w, b_eff = torch.zeros(3, 164, device=DEV), dev(c["views_w"]), dev(c["b_eff"])
    assert lib.danbo_train_cview(P(vin), 164, 161, P(views_w), P(b_eff), 3, P(out), stream()) == EINVAL
    torch.cuda.synchronize()
    assert (host(out) == SENT).all()


# ----------------------------------------------------------------------------- danbo_train_view_grads (+ head_chain's part sums)
def run_view_grads(lib, c, w, tag):
    """both routes of one case: atomics into a prefilled g_views_w, and the per-slice partial sums that head_chain adds up"""
    from core import hip_ops as ops
    rows, R, ch, n_codes = c["rows"], c["R"], c["view_ch"], c["n_codes"]
    rows_cap = rows + 5
    x = np.full(((rows_cap + 127) // 128 * 128, 128), np.nan, F32)                  # NaN in the padding rows behind cnt[4]
    x[:rows] = c["dpre"]
    frag = ops.FragBuffer.from_rows(dev(x))
    row_ray = np.full(rows_cap, 2 ** 30, np.int32)
    row_ray[:rows] = c["row_ray"]
    cnt = np.zeros(8, np.int32)
    cnt[4] = rows
    t_ray, t_cnt, t_vin, t_cam = dev(row_ray), dev(cnt), dev(c["vin"]), dev(c["cam_idx"])
    prefill = c["g_prefill"]
    want_dc, bnd_dc = ref.ray_grad_expect(c)                                        # n = the ray's rows
    results = []
    for route in ("atomic", "part"):
        d_cview = torch.zeros(R + 2, 128, device=DEV)
        d_cview[R:] = SENT
        csum = None
        if n_codes:
            csum = torch.zeros(n_codes + 1, 128, device=DEV)
            csum[n_codes:] = SENT
        g_views_w = dev(prefill)
        part = sent(ref.VG_SLICES * 128 * 160, value=float("nan")) if route == "part" else None
        call(lib, "danbo_train_view_grads", frag.data, t_ray, t_cnt, rows_cap, R, t_vin, c["ldv"], ch, t_cam, n_codes,
             d_cview, csum, g_views_w, part)
        dc = host(d_cview)
        assert (dc[R:] == SENT).all()
        w.check(tag + (route, "d_cview"), dc[:R], want_dc, bnd_dc)
        # second stage against float64 of the d cview the kernel itself wrote: its bound does not absorb the first stage's error
        gw, gw_bnd, cs, cs_bnd = ref.view_grad_expect(c, dc[:R], prefill[:, 256:])  # n = R + 32;  n = the camera's rays
        g = host(g_views_w)
        assert same(g[:, :256], prefill[:, :256])
        if n_codes:
            assert (host(csum)[n_codes:] == SENT).all()
            w.check(tag + (route, "csum"), host(csum)[:n_codes], cs, cs_bnd)
        if route == "atomic":
            w.check(tag + (route, "g_views_w"), g[:, 256:], gw, gw_bnd)             # += : the prefill is part of the sum
        else:
            assert same(g, prefill)                                                 # untouched until head_chain adds the slices up
            h = ref.head_chain_case(ch, 0, 0)
            outs = [sent(256, 256), sent(256), sent(128)]
            call(lib, "danbo_train_head_chain", h["g_wfv"], h["g_beff"], None, h["feature_w"], h["feature_b"],
                 h["views_w"], ch, 0, 0, 0, outs[0], outs[1], g_views_w, outs[2], None, part)
            g = host(g_views_w)
            w.check(tag + (route, "g_views_w"), g[:, 256:], gw, gw_bnd)
            w.check(tag + (route, "g_views_w[:, :256]"), g[:, :256], *ref.head_chain_expect(h)["g_views_w_a"])
        results.append((g[:, 256:].astype(F64), gw, gw_bnd))
    # the two routes agree within the sum of their bounds (each beside the float64 value of its own d cview)
    (ga, ra, ba), (gb, rb, bb) = results
    assert (np.abs((ga - ra) - (gb - rb)) <= ba + bb).all()


@pytest.mark.parametrize("rows", ref.VG_ROWS)
def test_view_grads_rows(lib, rows):
    """cnt[4] around the 8-row batches, the 16-row fragments and the 64-row chunks, with every row_ray pattern and view_ch"""
    w = Worst(f"view_grads rows={rows}")
    for case in ref.vg_cases_by_rows(rows):
        run_view_grads(lib, ref.view_grads_case(*case), w, case)
    w.done()


@pytest.mark.parametrize("R", ref.VG_R)
def test_view_grads_rays(lib, R):
    """R < 32: empty ray slices; 32: one ray each; 33 .. 261: the vector loop (8 rays) and its tail; every camera mode and view_ch"""
    w = Worst(f"view_grads R={R}")
    for case in ref.vg_cases_by_rays(R):
        run_view_grads(lib, ref.view_grads_case(*case), w, case)
    w.done()


def test_view_grads_more_rows_than_one_sweep_of_the_grid(lib, cu):
    """rows > 64 * 8 * cu: k_train_ray_grad's grid-stride loop iterates"""
    w = Worst("view_grads big")
    c = ref.vg_case_big(cu)
    assert c["rows"] > 64 * 8 * cu
    run_view_grads(lib, c, w, ("big",))
    w.done()


# ----------------------------------------------------------------------------- danbo_train_head_chain
@pytest.mark.parametrize("view_ch,n_codes,L_view", ref.HC_CASES)
def test_head_chain(lib, view_ch, n_codes, L_view):
    """What the step relies on: g_views_w[:, :256] is OVERWRITTEN (a NaN prefill leaves no trace), g_views_w[:, 256:] is
    ACCUMULATED into (left alone without vg_part, += the 32 slices with it)."""
    w = Worst(f"head_chain view_ch={view_ch} n_codes={n_codes}")
    c = ref.head_chain_case(view_ch, n_codes, L_view)
    exp = ref.head_chain_expect(c)           # n = 257 (start product + 256 fmas), 128 (sums over the view layer's rows), 0 (copy)
    ins = {k: dev(c[k]) for k in ("g_wfv", "g_beff", "csum", "feature_w", "feature_b", "views_w")}
    rng = ref.rng_of("hc part", view_ch)
    part_np = np.full((ref.VG_SLICES, 128, 160), np.nan, F32)
    part_np[:, :, :view_ch] = rng.normal(0.5, 0.5, size=(ref.VG_SLICES, 128, view_ch))
    for with_part in (False, True):
        prefill = c["g_prefill"].copy()
        prefill[:, :256] = np.nan
        g_views_w = dev(prefill)
        out = dict(g_feature_w=sent(256, 256), g_feature_b=sent(256), g_views_b=sent(128), g_codes=sent(n_codes * 16 + 4))
        call(lib, "danbo_train_head_chain", ins["g_wfv"], ins["g_beff"], ins["csum"] if n_codes else None, ins["feature_w"],
             ins["feature_b"], ins["views_w"], view_ch, n_codes, c["code_size"], c["code_col0"], out["g_feature_w"],
             out["g_feature_b"], g_views_w, out["g_views_b"], out["g_codes"] if n_codes else None,
             part_np if with_part else None)
        g = host(g_views_w)
        w.check("g_views_w[:, :256]", g[:, :256], *exp["g_views_w_a"])
        for k in ("g_feature_w", "g_feature_b", "g_views_b"):
            w.check(k, host(out[k]), *exp[k])
        codes = host(out["g_codes"])
        assert (codes[n_codes * 16:] == SENT).all()
        if n_codes:
            w.check("g_codes", codes[:n_codes * 16].reshape(n_codes, 16), *exp["g_codes"])
        if with_part:
            p64 = part_np[:, :, :view_ch].astype(F64)
            want, ab = prefill[:, 256:] + p64.sum(0), np.abs(prefill[:, 256:]) + np.abs(p64).sum(0)
            w.check("g_views_w[:, 256:]", g[:, 256:], want, ref.bound(ref.VG_SLICES + 1, ab))      # n = 33: 32 slices and the prefill
        else:
            assert same(g[:, 256:], prefill[:, 256:])
    w.done()


def test_head_chain_refuses_frame_code_columns_outside_the_view_inputs(lib):
    c = ref.head_chain_case(27, 4, 4)                                               # code_col0 = 27: 27 + 16 > view_ch = 27
    t = {k: dev(c[k]) for k in ("g_wfv", "g_beff", "csum", "feature_w", "feature_b", "views_w", "g_prefill")}
    outs = [sent(256, 256), sent(256), sent(128), sent(64)]
    rc = lib.danbo_train_head_chain(P(t["g_wfv"]), P(t["g_beff"]), P(t["csum"]), P(t["feature_w"]), P(t["feature_b"]), P(t["views_w"]), 27, 4, 16,
                                    27, P(outs[0]), P(outs[1]), P(t["g_prefill"]), P(outs[2]), P(outs[3]), None, stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and all((host(o) == SENT).all() for o in outs) and same(host(t["g_prefill"]), c["g_prefill"])


# ----------------------------------------------------------------------------- danbo_train_loss_grad
@pytest.mark.parametrize("R_index", range(5))
def test_loss_grad(lib, cu, R_index):
    """R around the 256 threads of a workgroup; 2 * 256 * cu + 37: more rays than the grid has threads"""
    R = ref.loss_rays(cu)[R_index]
    w = Worst(f"loss_grad R={R}")
    for mse in (0, 1):
        for bg_mode in ref.LOSS_BG:                # use_bg = 0; 1 with bgs; 1 with bgs = NULL (background 1)
            c = ref.loss_case(R, mse, bg_mode)     # w_fine != w_coarse, acc > 1 on some rays, every |e| >= 1e-4 or exactly 0
            out = dict(g_rgb=sent(R + 1, 3), g_acc=sent(R + 1), g_rgb0=sent(R + 1, 3), g_acc0=sent(R + 1))
            loss = torch.zeros(8, device=DEV)
            loss[2:] = SENT
            call(lib, "danbo_train_loss_grad", *(c[k] for k in ("rgb", "acc", "rgb0", "acc0", "target", "bgs")), c["use_bg"], R, mse,
                 c["w_fine"], c["w_coarse"], out["g_rgb"], out["g_acc"], out["g_rgb0"], out["g_acc0"], loss)
            grads, (want_loss, loss_bnd) = ref.loss_expect(c)
            for k, (want, bnd) in grads.items():
                got = host(out[k])
                assert (got[R:] == SENT).all()
                w.check((mse, bg_mode, k), got[:R], want, bnd)                      # n = 4
            got = host(loss)
            assert (got[2:] == SENT).all()
            w.check((mse, bg_mode, "loss"), got[:2], want_loss, loss_bnd)           # n = 3 R + 8
            if not c["use_bg"] and R > 5:
                assert not host(out["g_rgb"])[:5].any()                             # target == rgb exactly: gradient 0, L1 and MSE
    w.done()


# ----------------------------------------------------------------------------- danbo_train_draw_unmerge
@pytest.mark.parametrize("S,Sf", ref.DU_SHAPES)
def test_draw_unmerge(lib, cu, S, Sf):
    w = Worst(f"draw_unmerge S={S} Sf={Sf}")
    for R in ref.du_rays(cu):                      # 2 * 4 * cu + 37 rays: a wavefront owns several
        for bits_mode in ref.DU_BITS:
            c = ref.draw_unmerge_case(S, Sf, R, bits_mode)
            d_raw_c = dev(c["d_raw_c"])
            out = dict(d_raw_f=sent(R, Sf, 4), d_raw_rows=sent(R + 1, 4), label_c=sent(R, S, value=7, dtype=torch.uint8),
                       label_f=sent(R, Sf, value=7, dtype=torch.uint8))
            loss, maxabs = torch.zeros(8, device=DEV), torch.zeros(4, device=DEV)
            call(lib, "danbo_train_draw_unmerge", d_raw_c, *(c[k] for k in ("d_raw_sorted", "order", "bits_c", "bits_f", "weights", "alpha")),
                 R, S, Sf, out["d_raw_f"], out["d_raw_rows"], out["label_c"], out["label_f"], loss, maxabs)
            e = ref.draw_unmerge_expect(c)
            tag = (R, bits_mode)
            # copies, ONE fp32 addition per component, labels: bit for bit
            assert same(host(d_raw_c), e["d_raw_c"]), tag
            assert same(host(out["d_raw_f"]), e["d_raw_f"]), tag
            assert same(host(out["label_c"]), e["label_c"]) and same(host(out["label_f"]), e["label_f"]), tag
            rows = host(out["d_raw_rows"])
            assert (rows[R:] == SENT).all()
            w.check(tag + ("d_raw_rows",), rows[:R], *e["d_raw_rows"])              # n = S + Sf
            got_loss = host(loss)
            assert got_loss[2] == e["n_outside"] < 2 ** 24 and not got_loss[[0, 1, 3, 4, 5, 6, 7]].any(), tag
            want_max = max(e["maxabs_inside"], np.abs(rows[:R]).max())
            assert same(host(maxabs)[:1], np.array([want_max], F32)) and not host(maxabs)[1:].any(), tag
    w.done()


# ----------------------------------------------------------------------------- danbo_train_bone_lists
@pytest.mark.parametrize("rows", ref.BL_ROWS)
def test_bone_lists(lib, rows):
    """cnt[5] around the 64 lanes of a wavefront and the 256 rows of a workgroup; cnt[2] (the first importance row) at the first
    row, inside a wavefront and behind the last row"""
    for first in ref.BL_FIRST:
        for bits_mode in ref.BL_BITS:
            c = ref.bone_lists_case(rows, first, bits_mode)
            R, cap = c["R"], rows + 3
            cnt = np.zeros(8, np.int32)
            cnt[1], cnt[2], cnt[3], cnt[4], cnt[5] = c["n_c"], R + c["n_c"], c["n_f"], R + rows, rows
            lists, cntb = sent(24, cap, value=-1, dtype=torch.int32), torch.zeros(24, dtype=torch.int32, device=DEV)
            call(lib, "danbo_train_bone_lists", c["bits_c"], c["bits_f"], c["row_sample"], cnt, R, cap, lists,
                 cntb)
            sets, want_cnt = ref.bone_lists(c["bits_c"], c["bits_f"], c["row_sample"], R, c["n_c"], c["n_f"])
            got, got_cnt = host(lists), host(cntb)
            assert same(got_cnt, want_cnt), (first, bits_mode, got_cnt, want_cnt)
            for j in range(24):
                head = got[j, :want_cnt[j]].tolist()
                assert len(set(head)) == len(head) and set(head) == sets[j], (first, bits_mode, j)     # no duplicates, the same rows
                assert (got[j, want_cnt[j]:] == -1).all(), (first, bits_mode, j)                       # nothing behind the list
            if rows > 37 and first == "middle":
                assert c["n_c"] % 64 and c["n_f"] > 0


# ----------------------------------------------------------------------------- danbo_small_matmul
@pytest.mark.parametrize("M,N,K", ref.SM_SHAPES)
def test_small_matmul(lib, M, N, K):
    w = Worst(f"small_matmul {M}x{N}x{K}")
    for with_bias in (False, True):
        c = ref.small_matmul_case(M, N, K, with_bias)
        want, bnd = ref.small_matmul_expect(c)     # 2^-24 |ref| (ONE rounding) + K 2^-53 sum |terms| (the float64 sum)
        for a_t in (False, True):                  # the operand stored transposed: the other stride order
            for b_t in (False, True):
                A = dev(c["A"].T.copy() if a_t else c["A"])
                B = dev(c["B"].T.copy() if b_t else c["B"])
                sa = (1, M) if a_t else (K, 1)     # (stride over m, stride over k)
                sb = (1, K) if b_t else (N, 1)     # (stride over k, stride over n)
                ldc = N + 3
                C = sent(M, ldc)
                call(lib, "danbo_small_matmul", A, sa[0], sa[1], B, sb[0], sb[1], c["bias"], M, N, K, C, ldc)
                got = host(C)
                assert (got[:, N:] == SENT).all()                                   # the pad columns of C are left alone
                w.check((with_bias, a_t, b_t), got[:, :N], want, bnd)
    w.done()
