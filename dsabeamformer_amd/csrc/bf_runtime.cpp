// bf_runtime.cpp -- the C-ABI of libdsabf.so (include/dsabf.h): errors, the handle, weights, events, timers, the caller-stream calls.
//
// This is the thin host layer the reference keeps inline in main() (src/beamformer.cu:159-320,560-618):
// one transfer queue + n_streams compute queues, a device ring of n_blocks_on_gpu PSRDADA-sized blocks, one
// detected-power buffer per compute queue.  There is no CPU fallback: without a gfx950 device every compute
// entry point fails with BF_ERR_NO_DEVICE / BF_ERR_DEVICE.  The compute queues are bf_queues.cpp, the DM-trial stage
// bf_dm_stream.cpp, the measurement ABI (include/dsabf_bench.h) bf_bench_abi.cpp.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "bf_host_internal.h"
#include "bf_runtime_internal.h"
#include "ib/bf_incoherent.h"

// ---- what every stage shares (bf_runtime_internal.h): its device resources here, its lifetime (orphaned, stage_*) below
void* bf_resources::alloc(size_t bytes, bool zeroed, bool on_host)
{
    void* p = nullptr;
    if (err == hipSuccess) err = on_host ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (err != hipSuccess) return nullptr;
    (on_host ? pinned : device).push_back(p);
    if (zeroed) err = hipMemset(p, 0, bytes);
    return p;
}

void bf_resources::event(hipEvent_t* e)
{
    if (err == hipSuccess) err = hipEventCreateWithFlags(e, hipEventDisableTiming);
    if (err == hipSuccess) events.push_back(*e);
}

void bf_resources::queue(hipStream_t* q)
{
    if (err == hipSuccess) err = hipStreamCreateWithFlags(q, hipStreamNonBlocking);
    if (err == hipSuccess) queues.push_back(*q);
}

void bf_resources::device_sync()
{
    if (err == hipSuccess) err = hipDeviceSynchronize();
}

void bf_resources::wait()
{
    for (hipEvent_t e : events) (void)hipEventSynchronize(e);
    for (hipStream_t q : queues) (void)hipStreamSynchronize(q);
}

void bf_resources::release()
{
    wait();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    for (hipStream_t q : queues) (void)hipStreamDestroy(q);
    for (void* p : device) (void)hipFree(p);
    for (void* p : pinned) (void)hipHostFree(p);
    *this = bf_resources();
}

namespace dsabf::rt {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int orphaned(const bf_stage* s) { return s->h ? BF_OK : fail(BF_ERR_STATE, "the handle of this %s has been destroyed", s->noun); }

int stage_adopt(bf_stage* s, const char* who)
{
    s->h->stages.push_back(s);
    const hipError_t e = s->res.err;
    if (e == hipSuccess) return BF_OK;
    stage_destroy(s);
    return fail(BF_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
}

void stage_release(bf_stage* s)
{
    s->release_device();
    s->h = nullptr;
}

int stage_destroy(bf_stage* s)
{
    if (!s) return BF_OK;
    if (s->feeder) dm_stream_drop(s->feeder, s);
    if (s->h) {   // (NULL: the handle went first and took the device side with it)
        DeviceScope dev_scope_(s->h->device);
        std::vector<bf_stage*>& all = s->h->stages;
        all.erase(std::remove(all.begin(), all.end(), s), all.end());
        stage_release(s);
    }
    delete s;
    return BF_OK;
}

static int check_cfg(const bf_config* c)
{
    if (!c) return fail(BF_ERR_INVALID, "config is NULL");
    if (c->n_beams <= 0 || c->n_ant <= 0 || c->n_freq <= 0 || c->n_pol <= 0 || c->n_avg <= 0 ||
        c->n_out_per_gemm <= 0 || c->n_gemms_per_block <= 0 || c->n_blocks_on_gpu <= 0 || c->n_streams <= 0)
        return fail(BF_ERR_INVALID, "every geometry field must be positive");
    if (c->n_beams % 4) return fail(BF_ERR_INVALID, "N_BEAMS must be divisible by 4");       // src/beamformer.hh:155
    if (c->n_ant % 4) return fail(BF_ERR_INVALID, "N_ANTENNAS must be divisible by 4");      // src/beamformer.hh:156
    if (c->detect_mode != BF_DETECT_CANONICAL && c->detect_mode != BF_DETECT_FAST && c->detect_mode != BF_DETECT_CONTRACTED)
        return fail(BF_ERR_INVALID, "detect_mode must be BF_DETECT_CANONICAL, BF_DETECT_CONTRACTED or BF_DETECT_FAST");
    return BF_OK;
}

static dsabf::Geometry make_geom(const bf_config& c)
{
    dsabf::Geometry g{};
    g.n_beams = c.n_beams;
    g.n_ant = c.n_ant;
    g.n_freq = c.n_freq;
    g.n_ipo = c.n_pol * c.n_avg;
    g.n_out = c.n_out_per_gemm;
    g.n_time = g.n_out * g.n_ipo;
    g.n_ctiles = (c.n_beams + 15) / 16;
    g.fast_detect = c.detect_mode == BF_DETECT_FAST;
    g.contracted_detect = c.detect_mode == BF_DETECT_CONTRACTED;
    dsabf::read_env_switches(g);
    return g;
}

int supported_geom(const bf_config* c, dsabf::Geometry& g)
{
    if (int rc = check_cfg(c)) return rc;
    g = make_geom(*c);
    const char* why = nullptr;
    return dsabf::fused_supported(g, &why) ? BF_OK : fail(BF_ERR_INVALID, "unsupported geometry: %s", why);
}

}  // namespace dsabf::rt

int dsabf::set_error(int code, const char* msg)
{
    g_err = msg ? msg : "";
    return code;
}

extern "C" {

const char* bf_last_error(void) { return g_err.c_str(); }
#ifndef DSABF_KERNEL_BUILD_ID
#define DSABF_KERNEL_BUILD_ID "unknown"   // build.py: a hash over the kernel sources and their flags (build.kernel_build_id())
#endif
const char* bf_version(void) { return "dsabf 0.3 (gfx950, fused expand+int8 MFMA+detect; kernels " DSABF_KERNEL_BUILD_ID ")"; }

int bf_config_default(bf_config* cfg, int debug)
{
    if (!cfg) return fail(BF_ERR_INVALID, "config is NULL");
    cfg->n_beams = 256;
    cfg->n_ant = 64;
    cfg->n_freq = 256;
    cfg->n_pol = 2;
    cfg->n_avg = debug ? 1 : 16;
    cfg->n_out_per_gemm = 8;
    cfg->n_gemms_per_block = 32;
    cfg->n_blocks_on_gpu = 8;
    cfg->n_streams = 8;
    cfg->verbose = 0;
    cfg->detect_mode = BF_DETECT_CANONICAL;
    return BF_OK;
}

int bf_n_inputs_per_output(const bf_config* c) { return c ? c->n_pol * c->n_avg : 0; }
int bf_n_timesteps_per_gemm(const bf_config* c) { return c ? c->n_out_per_gemm * c->n_pol * c->n_avg : 0; }
size_t bf_bytes_per_gemm(const bf_config* c)
{
    return c ? (size_t)c->n_ant * c->n_freq * (size_t)bf_n_timesteps_per_gemm(c) : 0;
}
size_t bf_bytes_per_block(const bf_config* c) { return c ? bf_bytes_per_gemm(c) * (size_t)c->n_gemms_per_block : 0; }
size_t bf_floats_per_detect(const bf_config* c)
{
    return c ? (size_t)c->n_out_per_gemm * c->n_freq * (size_t)c->n_beams : 0;
}

int bf_device_count(int* count)
{
    if (!count) return fail(BF_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(BF_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return BF_OK;
}

int bf_device_name(int device, char* buf, size_t buflen)
{
    if (!buf || !buflen) return fail(BF_ERR_INVALID, "buffer is NULL");
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return BF_OK;
}

int bf_create(const bf_config* cfg, int device, bf_handle** out)
{
    if (!out) return fail(BF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    dsabf::Geometry g{};
    if (int rc = supported_geom(cfg, g)) return rc;

    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(BF_ERR_NO_DEVICE, "no HIP device visible (libdsabf has no CPU fallback)");
    if (device < 0 || device >= n) return fail(BF_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    DeviceScope dev_scope_(device);
    if (dev_scope_.err != hipSuccess) return fail(BF_ERR_DEVICE, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(dev_scope_.err));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(BF_ERR_NO_DEVICE, "device %d is %s; libdsabf is built for gfx950 only", device, prop.gcnArchName);

    bf_handle* h = new (std::nothrow) bf_handle();
    if (!h) return fail(BF_ERR_DEVICE, "out of host memory");
    h->cfg = *cfg;
    h->geom = g;
    h->device = device;
    h->n_cus = prop.multiProcessorCount;
    *out = h;  // from here on bf_destroy cleans up partial state

#define CREATE_TRY(expr)                                                                                     \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess) {                                                                              \
            bf_destroy(h);                                                                                   \
            *out = nullptr;                                                                                  \
            return fail(BF_ERR_DEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));                       \
        }                                                                                                    \
    } while (0)

    CREATE_TRY(hipMalloc(&h->d_wimage, dsabf::weight_image_bytes(g)));
    if (dsabf::weight_pair_image_bytes(g)) CREATE_TRY(hipMalloc(&h->d_wimage_p, dsabf::weight_pair_image_bytes(g)));
    if (dsabf::weight_fold_image_bytes(g)) CREATE_TRY(hipMalloc(&h->d_wimage_f, dsabf::weight_fold_image_bytes(g)));
    CREATE_TRY(hipMalloc((void**)&h->d_flag, 3 * sizeof(int)));
    CREATE_TRY(hipMalloc((void**)&h->d_data, bf_bytes_per_block(cfg) * (size_t)cfg->n_blocks_on_gpu));
    CREATE_TRY(hipMalloc((void**)&h->d_out, bf_floats_per_detect(cfg) * sizeof(float) * (size_t)cfg->n_streams));
    CREATE_TRY(hipMalloc((void**)&h->d_ded, (size_t)cfg->n_beams * sizeof(float) * (size_t)cfg->n_streams));
    // src/beamformer.cu:291-298: the reference zeroes its buffers
    CREATE_TRY(hipMemset(h->d_data, 0, bf_bytes_per_block(cfg) * (size_t)cfg->n_blocks_on_gpu));
    CREATE_TRY(hipMemset(h->d_out, 0, bf_floats_per_detect(cfg) * sizeof(float) * (size_t)cfg->n_streams));
    CREATE_TRY(hipMemset(h->d_ded, 0, (size_t)cfg->n_beams * sizeof(float) * (size_t)cfg->n_streams));
    CREATE_TRY(hipStreamCreateWithFlags(&h->h2d, hipStreamNonBlocking));
    h->streams.resize(cfg->n_streams, nullptr);
    h->join.resize(cfg->n_streams, nullptr);
    h->last_out.resize(cfg->n_streams, nullptr);
    h->last_q.resize(cfg->n_streams, 0);
    h->qbuf.resize(cfg->n_streams);
    for (int i = 0; i < cfg->n_streams; i++) {
        h->last_out[i] = h->d_out + bf_floats_per_detect(cfg) * (size_t)i;
        h->last_q[i] = i;
    }
    {
        const char* env = getenv("DSABF_COALESCE");
        h->coalesce = !(env && env[0] == '0');
    }
    CREATE_TRY(hipEventCreateWithFlags(&h->flush_done, hipEventDisableTiming));
    for (int i = 0; i < cfg->n_streams; i++) {
        CREATE_TRY(hipStreamCreateWithFlags(&h->streams[i], hipStreamNonBlocking));
        CREATE_TRY(hipEventCreateWithFlags(&h->join[i], hipEventDisableTiming));
    }
#undef CREATE_TRY
    return BF_OK;
}

int bf_destroy(bf_handle* h)
{
    if (!h) return BF_OK;
    DeviceScope dev_scope_(h->device);
    // gemm-units queued but never joined by an event or a sync: launch them (as the literal pattern would have) so that their
    // host copies land before the queues are drained below -- a destroy must not silently drop work that was accepted
    if (!h->streams.empty() && h->streams[0] && h->flush_done) (void)flush_units(h);
    h->pending.clear();
    for (auto s : h->streams)
        if (s) (void)hipStreamSynchronize(s);
    if (h->h2d) (void)hipStreamSynchronize(h->h2d);
    for (auto e : h->join)
        if (e) (void)hipEventDestroy(e);
    for (auto s : h->streams)
        if (s) (void)hipStreamDestroy(s);
    if (h->h2d) (void)hipStreamDestroy(h->h2d);
    if (h->flush_done) (void)hipEventDestroy(h->flush_done);
    if (h->t0) (void)hipEventDestroy(h->t0);
    if (h->t1) (void)hipEventDestroy(h->t1);
    for (void* p : std::initializer_list<void*>{h->d_wimage, h->d_wimage_p, h->d_wimage_f, h->d_flag, h->d_data, h->d_out, h->d_ded}) (void)hipFree(p);
    for (bf_stage* st : h->stages) stage_release(st);   // a stage that outlives its handle is left empty, not dangling
    h->dm_last = {};
    for (auto& sc : h->dm_scratch) (void)hipFree(sc.second);
    for (auto& b : h->qbuf)
        for (float* p : {b.out_blk, b.full_blk, b.stage_blk, b.ded_blk}) (void)hipFree(p);
    delete h;
    return BF_OK;
}

int bf_get_config(const bf_handle* h, bf_config* cfg)
{
    if (!h || !cfg) return fail(BF_ERR_INVALID, "NULL argument");
    *cfg = h->cfg;
    return BF_OK;
}

static int finish_weights(bf_handle* h, const int8_t* d_w, hipStream_t s)
{
    if (int rc = flush_units(h)) return rc;   // gemm-units still queued were enqueued under the OLD weights: launch them first
    for (auto q : h->streams) HIP_TRY(hipStreamSynchronize(q));   // ... and let them finish before the images change
    HIP_TRY(hipMemsetAsync(h->d_flag, 0, 3 * sizeof(int), s));
    HIP_TRY(dsabf::launch_weight_relayout(h->geom, d_w, h->d_wimage, h->d_wimage_p, h->d_wimage_f, h->d_flag, s));
    int bad[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(bad, h->d_flag, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->geom.paired = h->geom.fold = false;
    if (bad[0]) {
        h->weights_set = false;
        return fail(BF_ERR_INVALID, "weights contain an imaginary part of -128 (must be >= -127)");
    }
    // Beam sets symmetric about the boresight (the reference's linear fan and grid) have W[B-1-b] = conj(W[b]) exactly;
    // the device check above decides per weight set; DSABF_PAIRED=0 in the environment, or bf_set_switch(h, "paired", 0) before
    // the weights are set, forces the general kernel.
    const char* env = getenv("DSABF_PAIRED");   // read per weight set (not per launch): the choice is part of setting weights
    const bool general_only = h->force_general || (env && env[0] == '0');
    h->geom.paired = h->d_wimage_p != nullptr && bad[1] == 0 && !general_only;
    // Arrays that are point-symmetric about their phase centre (any regular line or grid) have W[A-1-a] = conj(W[a]) exactly: the
    // antenna-fold kernel then takes the place of either kernel (same bits).  bf_set_switch(h, "fold", 0), or DSABF_PAIRED=pair in
    // the environment (the profile refresh measures the conjugate-pair kernel through it), keeps the choice above.
    const bool pair_only = h->no_fold || (env && !strcmp(env, "pair"));
    h->geom.fold = h->d_wimage_f != nullptr && bad[2] == 0 && !general_only && !pair_only;
    if (h->geom.fold && dsabf::fused_launch_shape(h->geom, 1, h->n_cus).lds_bytes > 48 * 1024) h->geom.fold = false;   // (an "lds_pad" beyond the fold launcher's 48 KiB)
    h->weights_set = true;
    return BF_OK;
}

int bf_set_weights(bf_handle* h, const int8_t* w)
{
    if (!h || !w) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    const size_t n = (size_t)h->cfg.n_freq * h->cfg.n_ant * h->cfg.n_beams * 2;
    int8_t* d_w = nullptr;
    HIP_TRY(hipMalloc((void**)&d_w, n));
    hipError_t e = hipMemcpy(d_w, w, n, hipMemcpyHostToDevice);
    int rc = BF_OK;
    if (e != hipSuccess)
        rc = fail(BF_ERR_DEVICE, "weight upload failed: %s", hipGetErrorString(e));
    else
        rc = finish_weights(h, d_w, h->streams[0]);
    (void)hipFree(d_w);
    return rc;
}

int bf_set_weights_device(bf_handle* h, const int8_t* d_w, void* hip_stream)
{
    if (!h || !d_w) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    return finish_weights(h, d_w, as_stream(hip_stream));
}

int bf_alloc_pinned(void** ptr, size_t nbytes)
{
    if (!ptr) return fail(BF_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    HIP_TRY(hipHostMalloc(ptr, nbytes, hipHostMallocDefault));
    return BF_OK;
}

int bf_free_pinned(void* ptr)
{
    if (!ptr) return BF_OK;
    HIP_TRY(hipHostFree(ptr));
    return BF_OK;
}

int bf_host_register(void* ptr, size_t nbytes)
{
    if (!ptr || !nbytes) return fail(BF_ERR_INVALID, "NULL argument");
    HIP_TRY(hipHostRegister(ptr, nbytes, hipHostRegisterDefault));
    return BF_OK;
}

int bf_host_unregister(void* ptr)
{
    if (!ptr) return BF_OK;
    HIP_TRY(hipHostUnregister(ptr));
    return BF_OK;
}

static int event_create_here(bf_event** ev)
{
    if (!ev) return fail(BF_ERR_INVALID, "ev is NULL");
    *ev = nullptr;
    bf_event* e = new (std::nothrow) bf_event();
    if (!e) return fail(BF_ERR_DEVICE, "out of host memory");
    hipError_t rc = hipEventCreateWithFlags(&e->ev, hipEventDisableTiming);  // src/observation_loop.hh:59-60
    if (rc != hipSuccess) {
        delete e;
        return fail(BF_ERR_DEVICE, "hipEventCreateWithFlags: %s", hipGetErrorString(rc));
    }
    *ev = e;
    return BF_OK;
}

// HIP binds an event to the device that is current when it is created, and it can only be recorded on that device's
// streams: events a handle's queues will record are created under the HANDLE's device, whatever the caller's is.
int bf_event_create_on(bf_handle* h, bf_event** ev)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    ON_DEVICE(h);
    return event_create_here(ev);
}

int bf_event_create(bf_event** ev) { return event_create_here(ev); }

int bf_event_destroy(bf_event* ev)
{
    if (!ev) return BF_OK;
    hipError_t rc = hipEventDestroy(ev->ev);
    delete ev;
    if (rc != hipSuccess) return fail(BF_ERR_DEVICE, "hipEventDestroy: %s", hipGetErrorString(rc));
    return BF_OK;
}

int bf_event_query(bf_event* ev)
{
    if (!ev) return fail(BF_ERR_INVALID, "ev is NULL");
    hipError_t rc = hipEventQuery(ev->ev);  // an event never recorded reports "done", as in CUDA
    if (rc == hipSuccess) return BF_OK;
    if (rc == hipErrorNotReady) return BF_NOT_READY;
    return fail(BF_ERR_DEVICE, "hipEventQuery: %s", hipGetErrorString(rc));
}

int bf_event_synchronize(bf_event* ev)
{
    if (!ev) return fail(BF_ERR_INVALID, "ev is NULL");
    HIP_TRY(hipEventSynchronize(ev->ev));
    return BF_OK;
}

int bf_submit_block(bf_handle* h, int slot, const void* host, size_t nbytes, bf_event* ev)
{
    if (!h || !host) return fail(BF_ERR_INVALID, "NULL argument");
    if (slot < 0 || slot >= h->cfg.n_blocks_on_gpu) return fail(BF_ERR_INVALID, "slot %d out of range", slot);
    const size_t block = bf_bytes_per_block(&h->cfg);
    if (nbytes > block) return fail(BF_ERR_INVALID, "nbytes %zu exceeds the block size %zu", nbytes, block);
    ON_DEVICE(h);
    HIP_TRY(hipMemcpyAsync(h->d_data + block * (size_t)slot, host, nbytes, hipMemcpyHostToDevice, h->h2d));
    if (ev) {
        HIP_TRY(hipEventRecord(ev->ev, h->h2d));
        ev->recorded = true;
    }
    return BF_OK;
}

int bf_record_transfer_event(bf_handle* h, bf_event* ev)
{
    if (!h || !ev) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    HIP_TRY(hipEventRecord(ev->ev, h->h2d));
    ev->recorded = true;
    return BF_OK;
}

int bf_timer_start(bf_handle* h)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    ON_DEVICE(h);
    if (!h->t0) HIP_TRY(hipEventCreate(&h->t0));
    if (!h->t1) HIP_TRY(hipEventCreate(&h->t1));
    HIP_TRY(hipEventRecord(h->t0, nullptr));
    return BF_OK;
}

int bf_timer_stop(bf_handle* h, float* ms)
{
    if (!h || !ms) return fail(BF_ERR_INVALID, "NULL argument");
    if (!h->t0) return fail(BF_ERR_STATE, "bf_timer_start has not been called");
    ON_DEVICE(h);   // t1 goes onto the handle's device's null stream, where t0 is
    FLUSH_UNITS(h);
    HIP_TRY(hipEventRecord(h->t1, nullptr));
    HIP_TRY(hipEventSynchronize(h->t1));
    HIP_TRY(hipEventElapsedTime(ms, h->t0, h->t1));
    return BF_OK;
}

int bf_beamform_device(bf_handle* h, const void* d_packed, int n_units, float* d_out, void* hip_stream)
{
    if (!h || !d_packed || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_units <= 0) return fail(BF_ERR_INVALID, "n_units must be positive");
    if (int rc = check_weights(h)) return rc;
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 15))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed and d_out must be 16-byte aligned (the kernel loads "
                                    "16-byte pieces and stores 16-byte groups of beams)");
    ON_DEVICE(h);
    return launch_detect(h, d_packed, n_units, d_out, as_stream(hip_stream));
}

int bf_incoherent_device(bf_handle* h, const void* d_packed, int n_units, float* d_out, size_t stride, void* hip_stream)
{
    if (!h || !d_packed || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_units <= 0 || !stride) return fail(BF_ERR_INVALID, "n_units and stride must be positive");
    if (!dsabf::incoherent_supported(h->geom.n_ant, h->geom.n_ipo))
        return fail(BF_ERR_INVALID, "incoherent beam: 128 * %d antennas * %d samples per output exceeds 2^24 (the sum would not convert to float exactly)",
                    h->geom.n_ant, h->geom.n_ipo);
    if (((uintptr_t)d_packed & 15) || ((uintptr_t)d_out & 3))
        return fail(BF_ERR_INVALID, "misaligned device pointer: d_packed must be 16-byte aligned, d_out 4-byte aligned");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_incoherent(h->geom.n_ant, h->geom.n_freq, h->geom.n_ipo, h->geom.n_out, d_packed, n_units, d_out, stride, h->n_cus,
                                     as_stream(hip_stream)));
    return BF_OK;
}

int bf_expand_device(bf_handle* h, const void* d_in, size_t nbytes, void* d_out, void* hip_stream)
{
    if (!h || !d_in || !d_out) return fail(BF_ERR_INVALID, "NULL argument");
    if (nbytes % 16 || ((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15))
        return fail(BF_ERR_INVALID, "expand needs 16-byte aligned pointers and a multiple of 16 bytes");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_expand(d_in, nbytes, d_out, as_stream(hip_stream)));
    return BF_OK;
}

int bf_gemm_device(bf_handle* h, const void* d_packed_unit, float* d_c, void* hip_stream)
{
    if (!h || !d_packed_unit || !d_c) return fail(BF_ERR_INVALID, "NULL argument");
    if (int rc = check_weights(h)) return rc;
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_gemm_only(h->geom, h->d_wimage, d_packed_unit, d_c, h->n_cus, as_stream(hip_stream)));
    return BF_OK;
}

int bf_dedisperse_device(bf_handle* h, const float* d_out_unit, float* d_ded, void* hip_stream)
{
    if (!h || !d_out_unit || !d_ded) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_dedisperse(h->geom, d_out_unit, d_ded, as_stream(hip_stream)));
    return BF_OK;
}

int bf_dedisperse_band_device(bf_handle* h, const float* d_out_unit, int n_freq_total, float* d_ded, void* hip_stream)
{
    if (!h || !d_out_unit || !d_ded) return fail(BF_ERR_INVALID, "NULL argument");
    if (n_freq_total <= 0) return fail(BF_ERR_INVALID, "n_freq_total must be positive");
    ON_DEVICE(h);
    dsabf::Geometry g = h->geom;
    g.n_freq = n_freq_total;
    HIP_TRY(dsabf::launch_dedisperse(g, d_out_unit, d_ded, as_stream(hip_stream)));
    return BF_OK;
}

}  // extern "C"
