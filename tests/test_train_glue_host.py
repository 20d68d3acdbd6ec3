"""CPU-only proof of tests/train_glue_ref.py, the float64 references tests/test_gpu_train_glue.py holds the training step's view
branch and row glue against:
  * the adjoints (ray_grad, view_grad, head_chain) and cview against torch.autograd of the UNMERGED forward (feature_linear ->
    views_linears.0 on cat[feat, PE, frame code]) in float64, and loss_grad against autograd of trainer.py's losses;
  * the scatter-style references (draw_unmerge, bone_lists) against entry-by-entry loops;
  * the error bounds of every GPU case, evaluated from the reference alone: small beside the output (<= 1e-3 of its largest
    magnitude), and exceeded by each of seven deliberately wrong references."""
import numpy as np
import pytest
import torch

import train_glue_ref as ref

F32, F64 = np.float32, np.float64


def t64(x, grad=False):
    return torch.tensor(np.asarray(x, F64), dtype=torch.float64, requires_grad=grad)


def close(a, b, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    err, scale = np.abs(a - b).max(), np.abs(b).max()
    assert err <= 1e-12 * scale and scale > 0, (what, err, scale)


# ----------------------------------------------------------------------------- forward / adjoint consistency
@pytest.mark.parametrize("L,n_codes,cam_mode", [(4, 4, "interleaved"), (4, 4, "out_of_range"), (4, 4, "cam_null"), (0, 0, "no_codes")])
def test_view_branch_adjoints_match_autograd_of_the_unmerged_forward(L, n_codes, cam_mode):
    rng = np.random.default_rng(L * 7 + n_codes)
    R, rows, Cf = 9, 40, 16
    nd = 3 * (1 + 2 * L)
    view_ch = nd + (Cf if n_codes else 0)
    y7 = rng.normal(size=(rows, 256))
    row_ray = rng.integers(-1, R + 1, size=rows)                       # clamped like the kernel's
    ray = np.clip(row_ray, 0, R - 1)
    codes = rng.normal(size=(n_codes, Cf)) if n_codes else None
    cam = {"interleaved": np.arange(R) % 4, "out_of_range": rng.integers(-2, 7, size=R), "cam_null": None, "no_codes": None}[cam_mode]
    vin, _ = ref.view_inputs(rng.normal(size=(R, 3)), L, view_ch, normalise=True, codes=codes, cam_idx=cam)
    W_f, b_f = rng.normal(size=(256, 256)) / 16, rng.normal(size=256)
    W_v, b_v = rng.normal(size=(128, 256 + view_ch)) / 16, rng.normal(size=128)
    d_pre = rng.normal(size=(rows, 128))
    # the unmerged forward, float64 torch
    tW_f, tb_f, tW_v, tb_v = t64(W_f, True), t64(b_f, True), t64(W_v, True), t64(b_v, True)
    parts = [t64(vin[:, :nd])]
    if n_codes:
        tcodes = t64(codes, True)
        camc = np.zeros(R, np.int64) if cam is None else np.clip(cam, 0, n_codes - 1)
        parts.append(tcodes[torch.tensor(camc)])
    tvin = torch.cat(parts, 1)
    feat = t64(y7) @ tW_f.T + tb_f
    pre = torch.cat([feat, tvin[torch.tensor(ray)]], 1) @ tW_v.T + tb_v
    (pre * t64(d_pre)).sum().backward()
    # the merged form: pre_v = W_fv y7 + cview[ray]
    b_eff = b_v + W_v[:, :256] @ b_f
    cv, _ = ref.cview(vin, W_v, b_eff, view_ch)
    close(y7 @ (W_v[:, :256] @ W_f).T + cv[ray], pre.detach().numpy(), "pre_v")
    # its adjoint chain, from the same d pre_v, d W_fv = d pre_v^T y7 and d b_eff
    d_cview, _, _ = ref.ray_grad(d_pre, row_ray, R)
    (gw_b, _), cs = ref.view_grad(d_cview, vin, view_ch, cam, n_codes)
    hc = ref.head_chain(d_pre.T @ y7, d_pre.sum(0), None if cs is None else cs[0], W_f, b_f, W_v, n_codes, Cf, nd)
    close(hc["g_feature_w"][0], tW_f.grad.numpy(), "d W_f")
    close(hc["g_feature_b"][0], tb_f.grad.numpy(), "d b_f")
    close(hc["g_views_w_a"][0], tW_v.grad.numpy()[:, :256], "d W_v[:, :256]")
    close(gw_b, tW_v.grad.numpy()[:, 256:], "d W_v[:, 256:]")
    close(hc["g_views_b"][0], tb_v.grad.numpy(), "d b_v")
    if n_codes:
        got, want = hc["g_codes"][0], tcodes.grad.numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(want).max() > 0 or cam_mode == "cam_null"


@pytest.mark.parametrize("mse", [0, 1])
@pytest.mark.parametrize("bg_mode", ref.LOSS_BG)
def test_loss_grad_matches_autograd_of_the_trainer_losses(mse, bg_mode):
    c = ref.loss_case(257, mse, bg_mode)
    out, loss, _ = ref.loss_grad(c["rgb"], c["acc"], c["rgb0"], c["acc0"], c["target"], c["bgs"], c["use_bg"], mse, c["w_fine"], c["w_coarse"])
    R = c["R"]
    bg = t64(np.ones((R, 3)) if c["bgs"] is None else c["bgs"])
    for sfx, w, k in (("", c["w_fine"], 0), ("0", c["w_coarse"], 1)):
        rgb, acc = t64(c["rgb" + sfx], True), t64(c["acc" + sfx], True)
        pred = rgb + (1.0 - acc)[:, None] * bg if c["use_bg"] else rgb
        e = pred - t64(c["target"])
        term = ((e ** 2).mean() if mse else e.abs().mean()) * float(F32(w))
        term.backward()
        assert abs(float(term.detach()) - loss[k]) <= 1e-12 * abs(loss[k])
        close(out["g_rgb" + sfx][0], rgb.grad.numpy(), "g_rgb" + sfx)
        if c["use_bg"]:
            close(out["g_acc" + sfx][0], acc.grad.numpy(), "g_acc" + sfx)
        else:
            assert acc.grad is None and not out["g_acc" + sfx][0].any()
    if not c["use_bg"] and not mse:
        assert not out["g_rgb"][0][:5].any() and out["g_rgb"][0][5:].all()          # the exact-zero block gets gradient 0


# ----------------------------------------------------------------------------- the scatter-style references, entry by entry
def test_draw_unmerge_reference_equals_a_loop_over_the_samples():
    c = ref.draw_unmerge_case(5, 3, 4, "mixed")
    e = ref.draw_unmerge(c["d_raw_c"], c["d_raw_sorted"], c["order"], c["bits_c"], c["bits_f"], c["weights"], c["alpha"])
    S, Sf = 5, 3
    n_out = 0
    for r in range(c["R"]):
        row = np.zeros(4)
        assert sorted(c["order"][r]) == list(range(S + Sf))
        for i in range(S + Sf):
            src = c["order"][r, i]
            lab = int(float(c["weights"][r, i]) * float(c["alpha"][r, i]) > 0)
            if src < S:
                d = c["d_raw_sorted"][r, i] + c["d_raw_c"][r, src]
                assert d.dtype == F32 and np.array_equal(e["d_raw_c"][r, src], d) and e["label_c"][r, src] == lab
                outside = c["bits_c"][r, src] == 0
            else:
                d = c["d_raw_sorted"][r, i]
                assert np.array_equal(e["d_raw_f"][r, src - S], d) and e["label_f"][r, src - S] == lab
                outside = c["bits_f"][r, src - S] == 0
            if outside:
                row += d.astype(F64)
                n_out += lab
        assert np.abs(e["d_raw_rows"][0][r] - row).max() <= 1e-14
    assert e["n_outside"] == n_out > 0


def test_bone_lists_reference_on_a_hand_made_case():
    bits_c, bits_f = np.array([0b1, 0b110, 0], np.uint32), np.array([1 << 23, 0b11], np.uint32)
    row_sample = np.array([9, 9, 1, 0, 2, 1, 0], np.int32)             # R = 2; rows 2, 3, 4 coarse, rows 5, 6 importance
    sets, cntb = ref.bone_lists(bits_c, bits_f, row_sample, 2, 3, 2)
    assert sets[0] == {3, 5} and sets[1] == {2, 5} and sets[2] == {2} and sets[23] == {6}
    assert cntb.tolist() == [2, 2, 1] + [0] * 20 + [1]


# ----------------------------------------------------------------------------- the bounds: small beside the outputs ...
def small(b, r, what, rel=1e-3):
    b, r = np.asarray(b, F64), np.asarray(r, F64)
    assert np.isfinite(b).all() and np.isfinite(r).all() and (b >= 0).all(), what
    assert b.max(initial=0) <= rel * np.abs(r).max(initial=0), (what, b.max(), np.abs(r).max())


def test_bounds_of_view_inputs_cases_are_small():
    for L in ref.VI_L:
        for mode, G in ref.VI_MODES:
            for normalise in (0, 1):
                for code_mode in ref.VI_CODES:
                    for extra in (0, 8):
                        for R in ref.vi_rays(G):
                            r, b = ref.view_inputs_expect(ref.view_inputs_case(L, mode, G, normalise, code_mode, extra, R))
                            small(b, r, ("view_inputs", L, mode, G, normalise, code_mode, extra, R))


def test_bounds_of_cview_cases_are_small():
    for ch in ref.CVIEW_CH:
        for R in ref.cview_rays():
            r, b = ref.cview_expect(ref.cview_case(ch, R))
            small(b, r, ("cview", ch, R))


def vg_small(c, what):
    d, b = ref.ray_grad_expect(c)
    small(b, d, what + ("d_cview",))
    d32 = d.astype(F32)
    gw, gwb, cs, csb = ref.view_grad_expect(c, d32, c["g_prefill"][:, 256:])
    small(gwb, gw, what + ("g_views_w",))
    if cs is not None:
        small(csb, cs, what + ("csum",))


@pytest.mark.parametrize("rows", ref.VG_ROWS)
def test_bounds_of_view_grads_cases_by_rows_are_small(rows):
    for case in ref.vg_cases_by_rows(rows):
        vg_small(ref.view_grads_case(*case), case)


@pytest.mark.parametrize("R", ref.VG_R)
def test_bounds_of_view_grads_cases_by_rays_are_small(R):
    for case in ref.vg_cases_by_rays(R):
        vg_small(ref.view_grads_case(*case), case)


def test_bounds_of_the_large_view_grads_case_are_small():
    vg_small(ref.vg_case_big(), ("big",))


def test_bounds_of_head_chain_cases_are_small():
    for case in ref.HC_CASES:
        for k, (r, b) in ref.head_chain_expect(ref.head_chain_case(*case)).items():
            small(b, r, ("head_chain", case, k))


def test_bounds_of_loss_cases_are_small():
    for R in ref.loss_rays():
        for mse in (0, 1):
            for bg_mode in ref.LOSS_BG:
                grads, (loss, lb) = ref.loss_expect(ref.loss_case(R, mse, bg_mode))
                for k, (r, b) in grads.items():
                    small(b, r, ("loss_grad", R, mse, bg_mode, k))
                # The loss sums: every term is >= 0, so sum |terms| IS the sum and the bound is n 2^-24 of it, nothing to choose.
                # With the n = 3 R + 8 of the summation bound that is below 1e-3 up to R = 5 589; the largest case (R = 2 * 256 * cu
                # + 37, there to make the grid-stride loop iterate) has n 2^-24 = 2.3e-2 whatever its inputs are.
                n = 3 * R + 8
                assert np.allclose(lb, n * ref.U * loss * (1 + 1e-3), rtol=1e-12)
                small(lb, loss, ("loss", R, mse, bg_mode), rel=max(1e-3, n * ref.U * (1 + 1e-3) * (1 + 1e-9)))
                assert n * ref.U < 1e-3 or R == ref.loss_rays()[-1]


def test_bounds_of_draw_unmerge_cases_are_small():
    for S, Sf in ref.DU_SHAPES:
        for R in ref.du_rays():
            for bits_mode in ref.DU_BITS:
                e = ref.draw_unmerge_expect(ref.draw_unmerge_case(S, Sf, R, bits_mode))
                small(e["d_raw_rows"][1], e["d_raw_rows"][0], ("draw_unmerge", S, Sf, R, bits_mode))
                assert (bits_mode == "all_inside") == (not e["d_raw_rows"][0].any())
                assert e["n_outside"] < 2 ** 24                       # loss[2] is an exact integer


def test_bounds_of_small_matmul_cases_are_small():
    for shape in ref.SM_SHAPES:
        for with_bias in (False, True):
            r, b = ref.small_matmul_expect(ref.small_matmul_case(*shape, with_bias))
            small(b, r, ("small_matmul", shape, with_bias))


# ----------------------------------------------------------------------------- ... and exceeded by wrong references
def exceeds(wrong, r, b):
    return bool((np.abs(np.asarray(wrong, F64) - np.asarray(r, F64)) > b).any())


def test_a_view_column_shifted_by_one_exceeds_the_bound():
    c = ref.cview_case(27, 9)
    r, b = ref.cview_expect(c)
    w = c["views_w"].copy()
    w[:, 256:] = np.roll(w[:, 256:], 1, axis=1)
    assert exceeds(ref.cview(c["vin"], w, c["b_eff"], 27)[0], r, b)
    g = ref.view_grads_case(65, 33, 27, "long_runs", "sorted")
    d = ref.ray_grad_expect(g)[0].astype(F32)
    gw, gwb, _, _ = ref.view_grad_expect(g, d)
    assert exceeds(np.roll(gw, 1, axis=1), gw, gwb)


def test_sin_and_cos_swapped_exceeds_the_bound():
    c = ref.view_inputs_case(4, 1, 3, 1, "in_range", 0, 39)
    r, b = ref.view_inputs_expect(c)
    wrong = r.copy()
    for l in range(4):
        wrong[:, 3 + 6 * l:6 + 6 * l], wrong[:, 6 + 6 * l:9 + 6 * l] = r[:, 6 + 6 * l:9 + 6 * l], r[:, 3 + 6 * l:6 + 6 * l]
    assert exceeds(wrong, r, b)
    d = ref.view_inputs(c["rays_d"], 4, c["ldv"], c["skts"], 3, True)[1]
    assert np.allclose(r[:, 3:6], np.sin(d)) and np.allclose(r[:, 24:27], np.cos(8 * d))         # the kernel's column order


def test_the_last_row_of_a_ray_dropped_exceeds_the_bound():
    for pattern in ref.VG_PATTERNS:
        c = ref.view_grads_case(129, 33, 64, pattern, "no_codes")
        r, b = ref.ray_grad_expect(c)
        ray = np.clip(c["row_ray"], 0, c["R"] - 1)
        last = np.flatnonzero(ray == ray[50])[-1]
        keep = np.arange(c["rows"]) != last
        assert exceeds(ref.ray_grad(c["dpre"][keep], c["row_ray"][keep], c["R"])[0], r, b)


def test_the_bias_start_value_missing_exceeds_the_bound():
    for ch in ref.CVIEW_CH:
        c = ref.cview_case(ch, 9)
        r, b = ref.cview_expect(c)
        assert exceeds(ref.cview(c["vin"], c["views_w"], np.zeros(128), ch)[0], r, b)
    c = ref.head_chain_case(64, 4, 4)
    e = ref.head_chain_expect(c)
    wrong = ref.head_chain(c["g_wfv"], c["g_beff"], c["csum"], c["feature_w"], np.zeros(256), c["views_w"], 4, 16, 27)
    assert exceeds(wrong["g_views_w_a"][0], *e["g_views_w_a"])


def test_the_camera_off_by_one_exceeds_the_bound():
    c = ref.view_inputs_case(4, 0, 1, 1, "in_range", 0, 37)
    r, b = ref.view_inputs_expect(c)
    assert exceeds(ref.view_inputs(c["rays_d"], 4, c["ldv"], None, 1, True, c["codes"], c["cam_idx"] + 1)[0], r, b)
    for cam_mode in ("sorted", "interleaved", "out_of_range"):
        g = ref.view_grads_case(129, 33, 27, "long_runs", cam_mode)
        d = ref.ray_grad_expect(g)[0].astype(F32)
        _, _, cs, csb = ref.view_grad_expect(g, d)
        wrong = ref.view_grad(d, g["vin"], 27, g["cam_idx"] + 1, 4)[1][0]
        assert exceeds(wrong, cs, csb)
    h = ref.head_chain_case(64, 4, 4)
    e = ref.head_chain_expect(h)
    wrong = ref.head_chain(h["g_wfv"], h["g_beff"], np.roll(h["csum"], 1, axis=0), h["feature_w"], h["feature_b"], h["views_w"], 4, 16, 27)
    assert exceeds(wrong["g_codes"][0], *e["g_codes"])


def test_the_sign_of_one_minus_acc_flipped_exceeds_the_bound():
    for mse in (0, 1):
        for bg_mode in ("bgs", "bgs_null"):
            c = ref.loss_case(257, mse, bg_mode)
            grads, (loss, lb) = ref.loss_expect(c)
            flip = lambda a: 2.0 - np.asarray(a, F64)      # noqa: E731     1 - (2 - acc) = -(1 - acc)
            wrong, wloss, _ = ref.loss_grad(c["rgb"], flip(c["acc"]), c["rgb0"], flip(c["acc0"]), c["target"], c["bgs"], 1, mse, 1.0, 0.3)
            assert exceeds(wloss, loss, lb)
            assert exceeds(wrong["g_rgb"][0], *grads["g_rgb"]) and exceeds(wrong["g_rgb0"][0], *grads["g_rgb0"])
            assert exceeds(wrong["g_acc"][0], *grads["g_acc"])


def test_the_label_threshold_at_zero_included_exceeds_the_bound():
    c = ref.draw_unmerge_case(48, 16, 157, "mixed")
    e = ref.draw_unmerge_expect(c)
    one = np.ones_like(c["weights"])                                    # weights alpha >= 0 holds everywhere: every label set
    wrong = ref.draw_unmerge(c["d_raw_c"], c["d_raw_sorted"], c["order"], c["bits_c"], c["bits_f"], one, one)
    assert not np.array_equal(wrong["label_c"], e["label_c"]) and not np.array_equal(wrong["label_f"], e["label_f"])
    assert wrong["n_outside"] != e["n_outside"]
    prod = c["weights"].astype(F64) * c["alpha"].astype(F64)
    assert (prod == 0).any() and (prod[prod > 0] >= 1e-20).all() and (c["weights"] * c["alpha"] > 0).sum() == (prod > 0).sum()
