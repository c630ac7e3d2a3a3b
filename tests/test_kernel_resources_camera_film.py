"""Register budgets of the kernels of phip_camera_rays_device and phip_film_device (phip_camera_film.hip), read from the compiler as tests/test_kernel_resources.py
reads the others'; compile-only.

k_camera_rays is a streaming kernel -- a hash, the camera's matrix arithmetic, two 16-byte stores -- and k_film_values is k_film's gather with five accumulators:
neither has a reason to spill, so both are held to no scratch, and to the 128 VGPRs below which a 256-thread block keeps at least four waves per SIMD.
The (key, sample) pairs of phip_radiance_device add one by-value word and one branch to k_shade_r's sample source: its LDS-table builds must stay within the
absolute numbers tests/test_kernel_resources_radiance.py states for them (that file holds every build; the numbers are restated here for the object this change
is most likely to move)."""
import os

import pytest

from mitsuba_amd import _ffi
from test_kernel_resources import HIPCC, blocks_per_cu_by_sgprs, resources
from test_kernel_resources_radiance import launch_waves, rays_kernels

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


def test_camera_rays_and_the_film_gather_have_no_scratch():
    assert ("phip_camera_film.hip", [], "phip_camera_film.o") in _ffi.UNITS
    res = resources("phip_camera_film.hip")
    assert not any(name.startswith(("_Z6k_film", "_Z12k_film_tiled", "_Z12k_film_splat")) for name in res), list(res)      # the render's film kernels stay phip.hip's
    rays = [v for name, v in res.items() if name.startswith("_Z13k_camera_rays")]
    check = [v for name, v in res.items() if name.startswith("_Z21k_camera_pixels_check")]
    film = {name: v for name, v in res.items() if name.startswith("_Z13k_film_valuesILb")}
    assert len(rays) == 1 and len(check) == 1 and len(film) == 2, list(res)                                              # <false> and <true>
    for v in rays + check + list(film.values()):
        print(v)
        assert v["scratch"] == 0, v
        assert v["vgprs"] <= 128, v
        assert v["lds"] == 0, v


def test_ray_fed_vertex_kernels_keep_their_budgets_with_the_pairs():
    unit = next(u for u in _ffi.UNITS if u[2] == "phip_radiance0_0.o")
    ks = rays_kernels(resources(unit[0], unit[1]))
    seen = 0
    for (mm, strict, feat), v in ks.items():
        if feat == 0:
            continue
        seen += 1
        assert v["vgprs"] <= (88 if mm == 0 else 96), ((mm, strict, feat), v)
        assert v["scratch"] <= (64 if (mm in (1, 2) and strict == 0) else 96), ((mm, strict, feat), v)
        assert 5 * v["lds"] <= 160 * 1024, ((mm, strict, feat), v)
        assert blocks_per_cu_by_sgprs(v["sgprs"]) >= launch_waves(mm, feat), ((mm, strict, feat), v)
    assert seen == 8                                                                   # 4 material sets x {both tables in LDS, the emitter table only}, no strictNormals
