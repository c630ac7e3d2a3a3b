/*
 * k_camera_film.h -- the kernels of phip_camera_rays_device and phip_film_device (phip_camera_film.hip): the two ends of a render as entry points.
 *
 *   k_camera_pixels_check  the caller's pixel list against the crop window, before anything is written: one word says whether an entry is out of range
 *   k_camera_rays          one lane per camera sample: the sample's position from the counter stream (streamJitter, k_pool.h), its ray from cameraRay (dv_scene.h) --
 *                          the two calls cameraSample (k_shade.h) makes when a slot starts a sample, without the clip to the scene that follows them there
 *   k_film_values<SIGNED>  ImageBlock::put on a caller's values: k_film's gather (k_film.h: one lane per film pixel, a fixed order, no float atomics, any radius)
 *                          with the sample buffer in [y][x][k] order in place of the path pool's ids -- every render block is there (no shards), so there is no
 *                          tile table either.  The position of a sample, the bitmap of its render block, the clipped footprint and the table look-up are k_film's
 *                          statements, one by one; SIGNED leaves the sign test out of the validity check.
 * PHIP_SAMPLER_CTR only: the other samplers address their streams by film coordinates (the host refuses them).
 */
#pragma once

/* flag: one word, zeroed; set to 1 when an entry of pixels[0 .. m) is not below `limit` */
__global__ __launch_bounds__(BLOCK) void k_camera_pixels_check(const uint32_t *pixels, uint32_t m, uint32_t limit, unsigned long long *flag) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const bool bad = i < m && pixels[i] >= limit;
    if (__ballot(bad) && __lane_id() == 0) atomicOr(flag, 1ull);
}

/* Sample i = (pixel i / spp of the list, sample rc.sppFirst + i mod spp): two 16-byte stores, and the 8-byte ones the caller asked for.  pixels == NULL: the list is
   0 .. n / spp - 1.  Every entry of the list is below film.width * film.height (k_camera_pixels_check). */
__global__ __launch_bounds__(BLOCK) void k_camera_rays(DevScene S, RenderConst rc, const uint32_t *pixels, uint32_t n, float4 *rays, uint2 *keys, float2 *positions) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t p = __umulhi(i, rc.sppMagic);                      /* floor(i / sppPass) or one less (decodeId, k_pool.h) */
    uint32_t k = i - p * rc.sppPass;
    if (k >= rc.sppPass) { k -= rc.sppPass; ++p; }
    k += rc.sppFirst;
    const uint32_t pixel = pixels ? pixels[p] : p;
    const uint32_t w = (uint32_t) S.film.width, py = pixel / w, px = pixel - py * w;
    const V2 jit = streamJitter<false>(rc, pixel, k);
    const float sx = (float) px + jit.x, sy = (float) py + jit.y;
    V3 o, d; float mint, maxt;
    cameraRay(S.cam, sx, sy, o, d, mint, maxt);
    rays[2 * (size_t) i] = make_float4(o.x, o.y, o.z, mint);
    rays[2 * (size_t) i + 1] = make_float4(d.x, d.y, d.z, maxt);
    if (keys) keys[i] = make_uint2(pixel, k);
    if (positions) positions[i] = make_float2(sx, sy);
}

/* values: film.height * film.width * rc.sppPass float4 in [y][x][k] order; out: film.height * film.width x 5 */
template <bool SIGNED>
__global__ __launch_bounds__(BLOCK) void k_film_values(DevScene S, RenderConst rc, const float4 *values, float *out, int accumulate, unsigned long long *invalidCount) {
    const DevFilm &F = S.film;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= F.width || y >= F.height) return;
    /* a sample of source pixel s lands at s + jitter - 0.5 in [s-0.5, s+0.5): it can reach x iff
       s > x - radius - 0.5 and s <= x + radius + 0.5 */
    const int sx0 = max((int) floorf((float) x - F.radius - 0.5f) + 1, 0), sx1 = min((int) floorf((float) x + F.radius + 0.5f), F.width - 1);
    const int sy0 = max((int) floorf((float) y - F.radius - 0.5f) + 1, 0), sy1 = min((int) floorf((float) y + F.radius + 0.5f), F.height - 1);
    float acc[5] = { 0, 0, 0, 0, 0 };
    unsigned long long invalid = 0;
    for (int sy = sy0; sy <= sy1; ++sy) {
        for (int sx = sx0; sx <= sx1; ++sx) {
            const int offX = (sx >> rc.tileShift) << rc.tileShift, offY = (sy >> rc.tileShift) << rc.tileShift;
            const int bw = min(F.blockSize, F.width - offX) + 2 * F.border, bh = min(F.blockSize, F.height - offY) + 2 * F.border;
            /* destination pixel in the source block's bitmap coordinates */
            const int dx = x - (offX - F.border), dy = y - (offY - F.border);
            if (dx < 0 || dy < 0 || dx >= bw || dy >= bh) continue;
            const bool own = sx == x && sy == y;                /* a rejected sample is counted once: by the lane of its own pixel */
            const uint32_t pixel = (uint32_t) sy * (uint32_t) F.width + (uint32_t) sx;
            const float4 *src = values + (size_t) pixel * rc.sppPass;
            for (uint32_t k = 0; k < rc.sppPass; ++k) {
                const V2 jit = streamJitter<false>(rc, pixel, k + rc.sppFirst);
                const float px = (float) sx + jit.x, py = (float) sy + jit.y;
                const float posx = px - 0.5f - (float) (offX - F.border), posy = py - 0.5f - (float) (offY - F.border);
                const int minx = max((int) ceilf(posx - F.radius), 0), maxx = min((int) floorf(posx + F.radius), bw - 1);
                const int miny = max((int) ceilf(posy - F.radius), 0), maxy = min((int) floorf(posy + F.radius), bh - 1);
                const bool covers = !(dx < minx || dx > maxx || dy < miny || dy > maxy);
                if (!covers && !own) continue;
                const float4 v = src[k];
                /* validity check of ImageBlock::put: reject non-finite / negative samples (imageblock.h:148-151); SIGNED: non-finite ones only */
                if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w)) || (!SIGNED && (v.x < 0 || v.y < 0 || v.z < 0 || v.w < 0))) {
                    if (own) ++invalid;
                    continue;
                }
                if (!covers) continue;
                const float wx = F.table[min((int) fabsf(((float) dx - posx) * F.scaleFactor), PHIP_FILTER_RESOLUTION)];
                const float wy = F.table[min((int) fabsf(((float) dy - posy) * F.scaleFactor), PHIP_FILTER_RESOLUTION)];
                const float w = wx * wy;
                acc[0] += w * v.x; acc[1] += w * v.y; acc[2] += w * v.z; acc[3] += w * v.w; acc[4] += w * 1.0f;
            }
        }
    }
    float *o = out + ((size_t) y * F.width + x) * 5;
    if (accumulate) { for (int i = 0; i < 5; ++i) o[i] += acc[i]; }
    else { for (int i = 0; i < 5; ++i) o[i] = acc[i]; }
    if (invalid) atomicAdd(invalidCount, invalid);
}
