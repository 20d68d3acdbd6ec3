"""The skeleton overlay on the GPU (danbo_skel_project / danbo_skel_draw, core.utils.skeleton_draw, run_render --render_skel): both
kernels against the independent restatement of tests/skel_ref.py bit for bit -- every image size, width, source type and edge case
--, guard words around every output, a second call, misaligned and non-contiguous sources, rejected arguments, the Python entries
and the entry point.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import skel_ref as ref
from helpers import DEV, EINVAL, ROOT, entry, same_bits

pytestmark = pytest.mark.gpu
F32 = np.float32
J = ref.J
N_GUARD = 64          # guard bytes / words on either side of an output


def stream_ptr():
    from core import _hip
    return _hip.stream()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def guarded(n, dtype, fill):
    """-> (whole device buffer with N_GUARD guard elements on either side, the view of the n payload elements)"""
    buf = torch.full((n + 2 * N_GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[N_GUARD:N_GUARD + n]


def intact(buf, fill):
    return bool((buf[:N_GUARD] == fill).all()) and bool((buf[-N_GUARD:] == fill).all())


def gpu_project(c):
    """the raw C call with guard words around ends -> ends [N,24,4] (numpy)"""
    kps, w2c, focals = dev(c["kps"]), dev(c["w2c"]), dev(c["focals"])
    centers = None if c["centers"] is None else dev(c["centers"])
    N = len(c["kps"])
    buf, ends = guarded(N * J * 4, torch.int32, 0x5AFEC0D)
    rc = entry("danbo_skel_project")(kps.data_ptr(), w2c.data_ptr(), focals.data_ptr(), c["focals"].shape[1],
                                     None if centers is None else centers.data_ptr(), N, c["H"], c["W"], ends.data_ptr(), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(buf, 0x5AFEC0D), "a guard word was overwritten"
    return ends.reshape(N, J, 4).cpu().numpy()


def gpu_draw(src, ends, table, w):
    """the raw C call on device tensors with guard bytes around dst -> [N,H,W,3] uint8 (numpy)"""
    N, H, W, _ = src.shape
    buf, dst = guarded(N * H * W * 3, torch.uint8, 0xA5)
    colours = dev(table)
    rc = entry("danbo_skel_draw")(src.data_ptr(), int(src.dtype == torch.float32), ends.data_ptr(), colours.data_ptr(), w, N, H, W,
                                  dst.data_ptr(), stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert intact(buf, 0xA5), "a guard byte was overwritten"
    return dst.reshape(N, H, W, 3).cpu().numpy()


@pytest.mark.parametrize("name", ref.CASES)
def test_kernels_equal_the_restatement_bitwise(name):
    c = ref.case(name)
    if name != "direct":
        assert same_bits(gpu_project(c), c["ends"])
    ends = dev(c["ends"])
    f, u = (dev(s) for s in ref.sources(name))
    for w in ref.WIDTHS:
        for src, is_float in ((f, True), (u, False)):
            got = gpu_draw(src, ends, ref.colours(), w)
            want = ref.expected(name, w, is_float)
            assert same_bits(got, want), (name, w, is_float, int((got != want).any(-1).sum()))
    assert same_bits(gpu_draw(u, ends, ref.colours(True), 3), ref.expected(name, 3, False, flip=True))
    assert same_bits(gpu_draw(f, ends, ref.colours(True), 2), ref.expected(name, 2, True, flip=True))


def test_two_calls_give_the_same_bytes():
    c = ref.case("3x33x128")
    assert same_bits(gpu_project(c), gpu_project(c))
    ends, f = dev(c["ends"]), dev(ref.sources("3x33x128")[0])
    first, second = gpu_draw(f, ends, ref.colours(), 8), gpu_draw(f, ends, ref.colours(), 8)      # one repeat, not a stress loop
    assert same_bits(first, second) and same_bits(first, ref.expected("3x33x128", 8, True))


@pytest.mark.parametrize("name", ["3x37x53", "1x64x64"])
def test_sources_and_outputs_at_odd_addresses(name):
    """a source and an output that start 1 .. 3 elements past an aligned address (bytes of a uint8 source and of the output, floats
    of a float32 source): the wide paths must not be taken where the address does not allow them"""
    c = ref.case(name)
    ends, table = dev(c["ends"]), dev(ref.colours())
    for is_float, host in ((True, ref.sources(name)[0]), (False, ref.sources(name)[1])):
        n = host.size
        for shift in (1, 2, 3):
            room = torch.zeros(n + 8, dtype=torch.float32 if is_float else torch.uint8, device=DEV)
            src = room[shift:shift + n].view(host.shape)
            src.copy_(dev(host))
            buf = torch.full((n + 2 * N_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
            dst = buf[N_GUARD + shift:N_GUARD + shift + n]
            rc = entry("danbo_skel_draw")(src.data_ptr(), int(is_float), ends.data_ptr(), table.data_ptr(), 3, *host.shape[:3],
                                          dst.data_ptr(), stream_ptr())
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert bool((buf[:N_GUARD + shift] == 0xA5).all()) and bool((buf[N_GUARD + shift + n:] == 0xA5).all())
            assert same_bits(dst.reshape(host.shape).cpu().numpy(), ref.expected(name, 3, is_float)), (is_float, shift)


def test_rejected_arguments_leave_the_outputs_untouched():
    c = ref.case("1x64x64")
    src, ends, table = dev(ref.sources("1x64x64")[0]), dev(c["ends"]), dev(ref.colours())
    out = torch.full((64 * 64 * 3,), 0xA5, dtype=torch.uint8, device=DEV)
    e_out = torch.full((J * 4,), 77, dtype=torch.int32, device=DEV)
    kps, w2c, focals = dev(c["kps"]), dev(c["w2c"]), dev(c["focals"])

    def draw(**kw):
        a = dict(src=src.data_ptr(), src_is_float=1, ends=ends.data_ptr(), colours=table.data_ptr(), width=3, N=1, H=64, W=64, dst=out.data_ptr())
        assert set(kw) <= set(a)
        a.update(kw)
        return entry("danbo_skel_draw")(*a.values(), stream_ptr())

    def project(**kw):
        a = dict(kps=kps.data_ptr(), w2c=w2c.data_ptr(), focals=focals.data_ptr(), focal_stride=1, centers=None, N=1, H=64, W=64, ends=e_out.data_ptr())
        assert set(kw) <= set(a)
        a.update(kw)
        return entry("danbo_skel_project")(*a.values(), stream_ptr())

    for kw in [dict(src=None), dict(ends=None), dict(colours=None), dict(dst=None), dict(width=0), dict(width=65), dict(H=0), dict(W=4097),
               dict(N=0), dict(src_is_float=2), dict(dst=src.data_ptr()), dict(dst=src.data_ptr() + 64), dict(src=src.data_ptr() + 2),
               dict(ends=ends.data_ptr() + 2)]:
        assert draw(**kw) == EINVAL, kw
    for kw in [dict(kps=None), dict(w2c=None), dict(focals=None), dict(ends=None), dict(focal_stride=3), dict(H=4097), dict(W=0), dict(N=0),
               dict(kps=kps.data_ptr() + 2)]:
        assert project(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((e_out == 77).all())
    # and the calls they were variations of are accepted
    centers = dev(c["centers"])
    assert draw() == 0 and project(centers=centers.data_ptr()) == 0
    torch.cuda.synchronize()
    assert same_bits(out.reshape(1, 64, 64, 3).cpu().numpy(), ref.expected("1x64x64", 3, True))
    assert same_bits(e_out.reshape(1, J, 4).cpu().numpy(), c["ends"])


def test_python_entries():
    from core.utils.skeleton_draw import draw_skeletons, draw_skeletons_3d, skeleton3d_to_2d
    for name in ("3x37x53", "3x33x128", "1x5x7"):
        c = ref.case(name)
        f, u = ref.sources(name)
        stride = c["focals"].shape[1]
        focals = c["focals"] if stride == 2 else c["focals"][:, 0]
        ends = skeleton3d_to_2d(dev(c["kps"]), c["c2ws"], c["H"], c["W"], focals, c["centers"])
        assert ends.dtype == torch.int32 and ends.is_cuda and same_bits(ends.cpu().numpy(), c["ends"])
        # numpy input equals device input, for both source types; the reference's defaults (width 3, no flip)
        for src, is_float in ((f, True), (u, False)):
            a = draw_skeletons_3d(src, c["kps"], c["c2ws"], c["H"], c["W"], focals, c["centers"])
            b = draw_skeletons_3d(dev(src), dev(c["kps"]), torch.tensor(c["c2ws"]), c["H"], c["W"], focals, c["centers"])
            assert a.is_cuda and a.dtype == torch.uint8 and torch.equal(a, b)
            assert same_bits(a.cpu().numpy(), ref.expected(name, 3, is_float))
        got = draw_skeletons(dev(u), ends, width=8, flip=True)
        assert same_bits(got.cpu().numpy(), ref.expected(name, 8, False, flip=True))
    # one focal for every frame, as a float
    c = ref.case("1x5x7")
    one = skeleton3d_to_2d(c["kps"], c["c2ws"], 5, 7, float(c["focals"][0, 0]))
    assert same_bits(one.cpu().numpy(), c["ends"])
    # a non-contiguous source is refused, and so are other shapes and types
    f = dev(ref.sources("3x37x53")[0])
    ends = dev(ref.case("3x37x53")["ends"])
    wide = torch.zeros(3, 37, 60, 3, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        draw_skeletons(wide[:, :, :53], ends)
    with pytest.raises(ValueError, match="contiguous"):
        draw_skeletons(f.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), ends)
    with pytest.raises(ValueError, match="float32 or uint8"):
        draw_skeletons(f.double(), ends)
    with pytest.raises(ValueError, match="ends"):
        draw_skeletons(f, ends[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        draw_skeletons(f, ends.cpu())
    from core import _hip
    with pytest.raises(_hip.HipError, match="invalid argument"):
        draw_skeletons(f, ends, width=65)


# ----------------------------------------------------------------------------- the entry point
def test_run_render_writes_the_overlay(tmp_path):
    import run_nerf
    import run_render
    from core.config import config_parser as nerf_config_parser, txt_to_argstring
    cfg = os.path.join(ROOT, "danbo-pytorch_amd", "configs", "surreal", "danbo_fast.txt")
    run_nerf.train(["--config", cfg, "--basedir", str(tmp_path), "--expname", "demo", "--syn_poses", "2", "--syn_cams", "2",
                    "--syn_res", "32", "--syn_rest_scale", "0.714", "--N_rand", "512", "--N_sample_images", "4", "--i_print", "10",
                    "--i_weights", "20", "--i_testset", "20", "--render_factor", "0", "--n_iters", "20"])
    log = tmp_path / "demo"
    base = ["--nerf_args", str(log / "args.txt"), "--ckptpath", str(log / "000020.tar"), "--dataset", "synthetic", "--entry", "val",
            "--outputdir", str(tmp_path / "out"), "--render_type", "val", "--render_res", "32", "32"]
    out = tmp_path / "out"
    run_render.run_render(base + ["--runname", "plain"])
    run_render.run_render(base + ["--runname", "skel", "--render_skel"])
    run_render.run_render(base + ["--runname", "dev", "--render_skel", "--eval", "--eval_device"])
    run_render.run_render(base + ["--runname", "wide", "--render_skel", "--skel_width", "1", "--skel_flip"])
    run_render.run_render(base + ["--runname", "none", "--render_skel", "--no_save"])
    assert not (out / "plain" / "skel.npy").exists() and not (out / "none" / "skel.npy").exists() and not (out / "none" / "image.npy").exists()
    image, acc = np.load(out / "plain" / "image.npy"), np.load(out / "plain" / "acc.npy")
    for run in ("skel", "dev", "wide"):
        assert same_bits(np.load(out / run / "image.npy"), image) and same_bits(np.load(out / run / "acc.npy"), acc)
    # what the entry point must have drawn: render_data's kp, render_poses, hwf and centers through the restatement
    args = run_render.config_parser().parse_args(base + ["--runname", "x"])
    nerf_args, _ = nerf_config_parser().parse_known_args(txt_to_argstring(args.nerf_args))
    data, _ = run_render.load_render_data(args, nerf_args, run_render.get_render_dataset(args, nerf_args, DEV))
    H, W, focals = data["hwf"]
    assert (H, W) == (32, 32) and image.shape == (len(data["kp"]), 32, 32, 3) and image.dtype == np.uint8
    focals = np.asarray(focals, F32).reshape(len(image), -1)
    u, v = ref.project_uv(data["kp"], ref.w2c_of(data["render_poses"]), focals, data["centers"], H, W)
    ends = ref.ends_from_uv(u, v)
    skel = np.load(out / "skel" / "skel.npy")
    want = ref.draw(image, ends, ref.colours(), 3)
    assert skel.dtype == np.uint8 and same_bits(skel, want)
    n_drawn = int((skel != image).any(-1).sum())
    print("run_render --render_skel: pixels that differ from image.npy:", n_drawn, "of", image[..., 0].size)
    assert n_drawn > 0
    assert same_bits(np.load(out / "dev" / "skel.npy"), skel)            # device frames, quantised in the draw: identical
    assert same_bits(np.load(out / "wide" / "skel.npy"), ref.draw(image, ends, ref.colours(True), 1))
    # --render_mesh: the flag does nothing
    run_render.run_render(base[:-5] + ["--render_type", "selected", "--selected_idxs", "1", "--runname", "mesh", "--render_mesh", "--mesh_res", "15",
                                       "--mesh_radius", "1.2", "--render_skel"])
    assert (out / "mesh" / "meshes" / "000.ply").exists() and not (out / "mesh" / "skel.npy").exists()
