"""Bone-assignment maps (--render_confd / --render_entropy), the part that needs no GPU: the argument checks of the two entry points
of csrc/k_partmap.hip return DANBO_EINVAL before any launch (their binding: tests/test_abi_binding.py), the wrappers refuse CPU
tensors, the command line knows the new flag, and the palette the kernel is handed is the one definition of the joint colours."""
import os

import numpy as np
import pytest
import torch

from helpers import ADDR as P, EINVAL, golden, hip_lib as _lib     # P: an address no check follows


def part_colors(confd=P, bits=None, lst=None, cnt=None, n=4, mode=0, valid_only=0, palette=P, rgb=P):
    return _lib().danbo_part_colors_fwd(confd, bits, lst, cnt, n, mode, valid_only, palette, rgb, None)


def composite_colors(rgb_a=P, rgb_b=P, bits_a=None, bits_b=None, idx=P, w=P, R=2, S=8, Sf=4, ray_list=None, ray_count=None, out=P):
    return _lib().danbo_composite_colors_fwd(rgb_a, rgb_b, bits_a, bits_b, idx, w, R, S, Sf, ray_list, ray_count, out, None)


@pytest.mark.parametrize("kw", [dict(mode=2), dict(mode=-1), dict(n=-1), dict(valid_only=1), dict(mode=1, valid_only=1),
                                dict(palette=None), dict(confd=None), dict(rgb=None), dict(confd=P + 4)])
def test_part_colors_rejects_before_any_launch(kw):
    assert part_colors(**kw) == EINVAL


def test_part_colors_of_no_rows_launches_nothing():
    assert part_colors(n=0) == 0
    assert part_colors(n=0, mode=1, palette=None) == 0          # the palette belongs to mode 0


@pytest.mark.parametrize("kw", [dict(S=257), dict(Sf=65), dict(S=0), dict(Sf=-1), dict(R=-1), dict(ray_list=P), dict(ray_count=P),
                                dict(rgb_a=None), dict(w=None), dict(out=None), dict(rgb_b=None),
                                dict(idx=None), dict(idx=None, rgb_b=None),                 # the identity form has no second part
                                dict(idx=None, rgb_b=None, Sf=0, S=321)])
def test_composite_colors_rejects_before_any_launch(kw):
    assert composite_colors(**kw) == EINVAL


def test_composite_colors_of_no_rays_launches_nothing():
    assert composite_colors(R=0) == 0
    assert composite_colors(R=0, S=256, Sf=64) == 0
    assert composite_colors(R=0, idx=None, rgb_b=None, Sf=0, S=320) == 0       # an already sorted row of 256 + 64 samples


def test_wrappers_raise_on_cpu_tensors():
    from core import hip_ops as ops
    confd, rgb = torch.zeros(4, 24), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.part_colors(confd, "confd", rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.part_colors(confd, "entropy", rgb)
    with pytest.raises(ValueError):
        ops.part_colors(confd, "colour", rgb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.composite_colors(torch.zeros(2, 4, 3), torch.zeros(2, 4))


def test_run_render_knows_part_valid_only():
    import run_render
    base = ["--nerf_args", "a", "--ckptpath", "c", "--dataset", "synthetic", "--entry", "val", "--runname", "r"]
    p = run_render.config_parser()
    a = p.parse_args(base)
    assert (a.render_confd, a.render_entropy, a.part_valid_only) == (False, False, False)
    a = p.parse_args(base + ["--render_confd", "--part_valid_only"])
    assert a.render_confd and a.part_valid_only and not a.render_entropy


def test_engine_rejects_an_unknown_part_map():
    from core.render_engine import RenderEngine
    assert RenderEngine._part_mode(None) is None and RenderEngine._part_mode("entropy") == "entropy"
    with pytest.raises(ValueError):
        RenderEngine._part_mode("parts")


def test_kernel_palette_is_the_one_definition():
    """The kernel has no palette of its own: it reads the [24,3] table ops.part_palette hands it, and that is joint_colours() --
    bit for bit the hex list of core/networks/misc.py, and the colours the reference gave the golden logits' arg-max bones."""
    from core import hip_ops as ops
    from core.networks import misc
    pal = ops.part_palette("cpu")
    assert pal.dtype == torch.float32 and tuple(pal.shape) == (24, 3) and pal.is_contiguous()
    assert torch.equal(pal, misc.joint_colours())
    want = np.array([[int(h[i:i + 2], 16) / 255.0 for i in (0, 2, 4)] for h in misc._JOINT_COLOURS_HEX], np.float64).astype(np.float32)
    assert np.array_equal(pal.numpy(), want)
    g = golden("confd_colours")
    arg = torch.tensor(g["confd"]).argmax(-1)
    assert np.array_equal(pal[arg].numpy(), g["confidence_rgb"])
    # no second copy of the colours in the kernel source or the header
    from helpers import ROOT
    for path in ("danbo-pytorch_amd/csrc/k_partmap.hip", "include/danbo_partmap.h"):
        text = open(os.path.join(ROOT, path)).read().lower()
        assert not any(h in text for h in ("4b0082", "ff8c00", "9acd32", "0.29411", "0.54901"))
