/*
 * host_multi.h -- host side of libphip.so, third of three: a render call on several GPUs.  The RCCL binding (dlopen at the first multi-GPU render), the kernel
 * that sums aliased films, and renderMultiDevice: one host thread + stream per GPU over the scene's replicas (ensureReplicas), the films merged on devices[0]
 * by one ncclReduce.  A device's failure is reported through setErr of the unit that includes this header.
 * Included by phip.hip alone, after host_render.h; k_add_films is the unit's last kernel ahead of the debug kernels (phip_debug.inl).
 */
#pragma once
#include "host_render.h"
#include <dlfcn.h>
#include <map>
#include <rccl/rccl.h>          /* types and prototypes only: librccl is bound with dlopen at the first multi-GPU render */

/* ---- RCCL, bound at the first multi-GPU render (librccl is not a load-time dependency of single-GPU users; a process that
   already carries an RCCL -- PyTorch does -- keeps exactly one copy) ---- */
namespace {
struct Rccl {
    void *handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::mutex lock;
    std::map<std::vector<int>, std::vector<ncclComm_t>> comms;       /* one communicator clique per device list, kept for the process */
    void bind() {
        if (handle) return;
        for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) { handle = dlopen(name, RTLD_NOW | RTLD_LOCAL); if (handle) break; }
        if (!handle) throw std::runtime_error(std::string("multi-GPU render needs librccl: ") + dlerror());
        auto sym = [&](const char *n) { void *s = dlsym(handle, n); if (!s) throw std::runtime_error(std::string("librccl lacks ") + n); return s; };
        CommInitAll = (decltype(CommInitAll)) sym("ncclCommInitAll"); CommDestroy = (decltype(CommDestroy)) sym("ncclCommDestroy");
        Reduce = (decltype(Reduce)) sym("ncclReduce"); GroupStart = (decltype(GroupStart)) sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd)) sym("ncclGroupEnd"); GetErrorString = (decltype(GetErrorString)) sym("ncclGetErrorString");
    }
    void check(ncclResult_t r, const char *what) { if (r != ncclSuccess) throw std::runtime_error(std::string(what) + ": " + (GetErrorString ? GetErrorString(r) : "RCCL error")); }
    const std::vector<ncclComm_t> &clique(const std::vector<int> &devices) {
        auto it = comms.find(devices);
        if (it != comms.end()) return it->second;
        std::vector<ncclComm_t> c(devices.size());
        check(CommInitAll(c.data(), (int) devices.size(), devices.data()), "ncclCommInitAll");
        return comms.emplace(devices, std::move(c)).first->second;
    }
};
Rccl g_rccl;

__global__ void k_add_films(float *dst, const float *src, size_t n) {
    const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
} // namespace

/* The call's shard on p->n_devices GPUs: one host thread + stream per device, blocks dealt round-robin in the reference's
   spiral order, films merged on devices[0] by one ncclReduce(sum) -- the in-process analogue of the reference's workers
   handing ImageBlocks to BlockedRenderProcess::processResult (renderproc.cpp:142-149). */
static int renderMultiDevice(phip_scene *sc, const phip_render_params *p, float *dOut, phip_stats *stats) {
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    const int n = p->n_devices;
    const bool alias = (p->flags & PHIP_FLAG_ALIAS_DEVICES) != 0;
    std::vector<int> devices(p->devices, p->devices + n);
    bool distinct = true;
    for (int i = 0; i < n; ++i) for (int j = 0; j < i; ++j) if (devices[j] == devices[i]) distinct = false;
    if (!distinct && !alias) throw std::invalid_argument("a device is listed twice (PHIP_FLAG_ALIAS_DEVICES allows it for tests)");
    if (const char *bad = ensureReplicas(sc, devices.data(), n)) throw std::invalid_argument(bad);
    const int W = sc->devs[0]->dev.film.width, H = sc->devs[0]->dev.film.height;
    const size_t filmFloats = (size_t) W * H * 5;
    const int S = p->shard_count > 0 ? p->shard_count : 1, s = p->shard_index;
    std::vector<float *> out(n, nullptr);
    out[0] = dOut;
    for (int i = 1; i < n; ++i) {
        SceneDev &sd = *sc->devs[i];
        HIP_TRY(hipSetDevice(sd.device));
        if (sd.film.n < filmFloats) sd.film.alloc(filmFloats);
        out[i] = sd.film.p;
    }
    std::vector<phip_stats> st(n);
    std::vector<int> rc(n, PHIP_OK);
    std::vector<std::string> err(n);
    std::vector<std::thread> workers;
    phip_render_params q = *p;
    q.flags &= ~PHIP_FLAG_SAMPLE_BUFFER;                         /* per-sample export is a single-device test hook */
    for (int i = 0; i < n; ++i) {
        workers.emplace_back([&, i]() {
            try {
                phip_render_params mine = q;
                if (i > 0) mine.flags &= ~PHIP_FLAG_ACCUMULATE;   /* only the root's buffer carries the previous calls */
                rc[i] = renderOnDevice(sc, *sc->devs[i], &mine, s + S * i, S * n, out[i], &st[i]);
            } catch (const std::invalid_argument &e) { rc[i] = PHIP_ERR_INVALID; err[i] = e.what(); }
              catch (const std::exception &e) { rc[i] = PHIP_ERR_DEVICE; err[i] = e.what(); }
        });
    }
    for (auto &w : workers) w.join();
    bool cancelled = false;
    for (int i = 0; i < n; ++i) {
        if (rc[i] == PHIP_ERR_CANCELLED) cancelled = true;
        else if (rc[i] != PHIP_OK) return setErr(rc[i], "device " + std::to_string(devices[i]) + ": " + err[i]);
    }
    /* ---- merge: film(devices[0]) += sum of the others ---- */
    const auto tr0 = clk::now();
    if (!cancelled) {
        if (distinct) {
            std::lock_guard<std::mutex> g(g_rccl.lock);
            g_rccl.bind();
            const std::vector<ncclComm_t> &comm = g_rccl.clique(devices);
            g_rccl.check(g_rccl.GroupStart(), "ncclGroupStart");
            for (int i = 0; i < n; ++i) {
                SceneDev &sd = *sc->devs[i];
                HIP_TRY(hipSetDevice(sd.device));
                g_rccl.check(g_rccl.Reduce(out[i], out[i], filmFloats, ncclFloat, ncclSum, 0, comm[i], sd.stream), "ncclReduce");
            }
            g_rccl.check(g_rccl.GroupEnd(), "ncclGroupEnd");
            for (int i = 0; i < n; ++i) { HIP_TRY(hipSetDevice(sc->devs[i]->device)); HIP_TRY(hipStreamSynchronize(sc->devs[i]->stream)); }
        } else {
            /* aliased devices (test hook): the films are in the same memory, a kernel sums them */
            HIP_TRY(hipSetDevice(devices[0]));
            for (int i = 1; i < n; ++i)
                hipLaunchKernelGGL(k_add_films, dim3((unsigned) ((filmFloats + 255) / 256)), dim3(256), 0, sc->devs[0]->stream, out[0], (const float *) out[i], filmFloats);
            HIP_TRY(hipStreamSynchronize(sc->devs[0]->stream));
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipSetDevice(devices[0]));
    if (stats) {
        phip_stats t; memset(&t, 0, sizeof(t));
        for (int i = 0; i < n; ++i) {
            const phip_stats &a = st[i];
            addWork(t, a);
            t.invalid_samples += a.invalid_samples; t.iterations = std::max(t.iterations, a.iterations);
            t.trace_kernel_ms = std::max(t.trace_kernel_ms, a.trace_kernel_ms); t.shadow_kernel_ms = std::max(t.shadow_kernel_ms, a.shadow_kernel_ms);
            t.shade_kernel_ms = std::max(t.shade_kernel_ms, a.shade_kernel_ms); t.film_kernel_ms = std::max(t.film_kernel_ms, a.film_kernel_ms);
            t.fused_kernel_ms = std::max(t.fused_kernel_ms, a.fused_kernel_ms);
            t.algorithmic_bytes += a.algorithmic_bytes; t.trace_kernel_bytes += a.trace_kernel_bytes; t.fused = i ? (t.fused & a.fused) : a.fused; t.vertex_traced |= a.vertex_traced;
        }
        t.n_devices = (uint32_t) n;
        t.reduce_ms = std::chrono::duration<double, std::milli>(clk::now() - tr0).count();
        t.render_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        *stats = t;
    }
    return cancelled ? PHIP_ERR_CANCELLED : PHIP_OK;
}
