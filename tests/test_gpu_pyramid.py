"""phip_mip_pyramid_device on the GPU: the levels are those of the host call phip_mip_pyramid bit for bit (tests/test_pyramid_host.py holds that one to the
reference), at the sizes where the kernels take another path -- one texel, one axis, no multiple of anything, the reference-built fixtures, and three sizes around
the bound of the single-block tail kernel (PYR_TAIL_LDS_BYTES = 65536: a level fits with its temporary and the next level when 12 * (w h + w' h + w' h') <= 65536)
-- with sentinels around every output level, and composed with update_appearance against scenes created from host-built levels.  Everything is compared as uint32."""
import numpy as np
import pytest

from mitsuba_amd import _abi as A, scene as S
from test_gpu_appearance import env_scene, textured_box
from test_gpu_parity import gpu  # noqa: F401  (the fixture)
from test_gpu_scene_update import render, same_bits
from test_pyramid_host import GOLDEN, WRAPS, image

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD, SENTINEL = 8, -77.25
TAIL_FLOATS = 65536 // 4


def tail_fits(w, h):
    tw, th = max(1, (w + 1) // 2), max(1, (h + 1) // 2)
    return 3 * (w * h + tw * h + tw * th) <= TAIL_FLOATS


@pytest.fixture(scope="module")
def gs(gpu, gauss):
    scene = gpu.Scene(S.cornell_box(16, 16, gauss).desc())
    yield scene
    scene.close()


def guarded_levels(torch, w, h, first=0):
    """one tensor per level inside a buffer with GUARD sentinel floats on either side: ([level views], [buffers])"""
    views, buffers = [], []
    for l, (lh, lw) in enumerate(S.pyramid_sizes(w, h)):
        if l < first:
            views.append(None); buffers.append(None)
            continue
        b = torch.full((3 * lh * lw + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        views.append(b[GUARD:GUARD + 3 * lh * lw].view(lh, lw, 3)); buffers.append(b)
    return views, buffers


def assert_levels(torch, got, buffers, want, what):
    for l, (g, b, w) in enumerate(zip(got, buffers, want)):
        if g is None:
            continue
        assert same_bits(g.cpu().numpy(), w), "%s: level %d differs from the host call's" % (what, l)
        if b is not None:
            edge = torch.cat([b[:GUARD], b[-GUARD:]]).cpu().numpy()
            assert (edge == SENTINEL).all(), "%s: level %d wrote outside its %d floats" % (what, l, w.size)


def device_against_host(torch, gs, img, wu, wv, maxv, what, **kw):
    want = S.mip_pyramid_lanczos(img, wu, wv, maxv)
    views, buffers = guarded_levels(torch, img.shape[1], img.shape[0])
    got = gs.mip_pyramid(torch.from_numpy(img).cuda(), wu, wv, maxv, out=views, **kw)
    assert_levels(torch, got, buffers, want, what)
    return want


# 40 x 24: level 0 fits the tail kernel; 97 x 63: level 1 (49 x 32) is the first that fits; 161 x 95: two full two-pass steps, level 2 (41 x 24) is the first
SIZES = [(1, 1), (2, 1), (1, 2), (3, 3), (25, 15), (64, 32), (40, 24), (97, 63), (161, 95)]


def test_the_three_sizes_sit_where_the_tail_bound_puts_them():
    assert tail_fits(40, 24)
    assert not tail_fits(97, 63) and tail_fits(49, 32)
    assert not tail_fits(161, 95) and not tail_fits(81, 48) and tail_fits(41, 24)


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("maxv", [1.0, INF], ids=["max1", "maxinf"])
def test_device_equals_host_call(gs, size, maxv):
    import torch
    w, h = size
    img = image(w, h, 7 * w + h, -0.25, 1.5 if maxv == 1.0 else 9.0e4, half_exact=False)
    device_against_host(torch, gs, img, "repeat" if maxv == INF else "mirror", "clamp" if maxv == INF else "repeat", maxv, "%dx%d" % size)


def test_every_wrap_mode_on_each_axis(gs):
    import torch
    img = image(13, 7, 5, -0.1, 1.2, half_exact=False)
    for wu in WRAPS:
        for wv in WRAPS:
            for maxv in (1.0, INF):
                device_against_host(torch, gs, img, wu, wv, maxv, "%s x %s, max %r" % (wu, wv, maxv))


def test_level0_not_written_written_apart_and_in_place(gs):
    import torch
    img = image(25, 15, 9, -0.5, 1.5, half_exact=False)
    want = S.mip_pyramid_lanczos(img, "clamp", "mirror", 1.0)
    assert not np.array_equal(want[0], img)                           # level 0 comes back clamped at 0 and rounded to half
    src = torch.from_numpy(img).cuda()
    views, buffers = guarded_levels(torch, 25, 15, first=1)           # d_levels[0] = NULL
    got = gs.mip_pyramid(src, "clamp", "mirror", 1.0, out=views)
    assert got[0] is None and same_bits(src.cpu().numpy(), img)
    assert_levels(torch, got, buffers, want, "level 0 not written")
    views, buffers = guarded_levels(torch, 25, 15)                    # a distinct level 0
    assert_levels(torch, gs.mip_pyramid(src, "clamp", "mirror", 1.0, out=views), buffers, want, "level 0 apart")
    assert same_bits(src.cpu().numpy(), img)
    views, buffers = guarded_levels(torch, 25, 15)                    # in place
    views[0][:] = src
    got = gs.mip_pyramid(views[0], "clamp", "mirror", 1.0, out=views)
    assert got[0] is views[0]
    assert_levels(torch, got, buffers, want, "level 0 in place")
    plain = gs.mip_pyramid(src, "clamp", "mirror", 1.0)               # no `out`: every level allocated
    assert_levels(torch, plain, [None] * len(plain), want, "allocated")


def test_on_the_callers_stream(gs):
    import torch
    img = image(64, 32, 3, 0.0, 2.0, half_exact=False)
    want = S.mip_pyramid_lanczos(img * np.float32(0.5), "repeat", "clamp", INF)
    stream = torch.cuda.Stream()
    base = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        src = base * 0.5                                              # the producer runs on the caller's stream; the call is ordered after it
        views, buffers = guarded_levels(torch, 64, 32)
        got = gs.mip_pyramid(src, "repeat", "clamp", INF, out=views, stream=stream)
    assert_levels(torch, got, buffers, want, "caller's stream")


@pytest.mark.parametrize("group", GOLDEN, ids=[g[1] for g in GOLDEN])
def test_reference_built_fixtures_come_out_as_stored(gs, group):
    import torch
    scene, key, kind, wu, wv, levels = group
    views, buffers = guarded_levels(torch, levels[0].shape[1], levels[0].shape[0])
    args = ("repeat", "clamp", INF) if kind == "envmap" else (wu, wv, 1.0)
    assert_levels(torch, gs.mip_pyramid(torch.from_numpy(levels[0]).cuda(), *args, out=views), buffers, levels, key)


# ---- composition: update_appearance from an "image" == a scene created from host-built Lanczos levels ----
PATHS = (0, A.PHIP_FLAG_NO_FUSED)


def lanczos_textures(sb):
    names = {v: k for k, v in S.WRAP_MODES.items()}
    for t in sb.textures:
        t["levels"] = S.mip_pyramid_lanczos(t["levels"][0], names[t["wrap_u"]], names[t["wrap_v"]], 1.0)
    return sb


@pytest.mark.parametrize("size", [(3, 5), (64, 64)], ids=["5x3", "64x64"])
def test_textures_from_an_image_tensor(gpu, gauss, size):
    import torch
    sb = textured_box(gauss, size)                                    # as created: other texels, the box stand-in's levels
    new = lanczos_textures(textured_box(gauss, size, seed=12))
    raw = [textured_box(gauss, size, seed=12).textures[i]["levels"][0] for i in range(2)]
    fresh, scene = gpu.Scene(new.desc()), gpu.Scene(sb.desc())
    texs = [dict(t) for t in new.textures]
    for t, img in zip(texs, raw):
        del t["levels"]
        t["image"] = torch.from_numpy(img).cuda()
    scene.update_appearance(textures=texs)
    integ = gpu.PathHIP(maxDepth=5)
    for flags in PATHS:
        got, want = render(gpu, scene, integ, 4, flags), render(gpu, fresh, integ, 4, flags)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], flags
    host = gpu.Scene(sb.desc())                                       # the same from a numpy image: the host call, host pointers
    host.update_appearance(textures=[dict(t, image=img) for t, img in zip(texs, raw)])
    got, want = render(gpu, host, integ, 4, 0), render(gpu, fresh, integ, 4, 0)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("size", [(8, 16), (130, 67)], ids=["16x8", "67x130"])
def test_environment_map_from_an_image_tensor(gpu, gauss, size):
    import torch
    sb, new = env_scene(gauss, size, 5), env_scene(gauss, size, 6)
    raw, scale, m, _ = new._envmap
    levels = S.mip_pyramid_lanczos(raw, "repeat", "clamp", INF)
    new._envmap = (levels[0], scale, m, levels)
    fresh, scene = gpu.Scene(new.desc()), gpu.Scene(sb.desc())
    scene.update_appearance(envmap=dict(image=torch.from_numpy(raw).cuda()))
    integ = gpu.PathHIP(maxDepth=5)
    for flags in PATHS:
        got, want = render(gpu, scene, integ, 4, flags), render(gpu, fresh, integ, 4, flags)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and got[2] == want[2], flags
