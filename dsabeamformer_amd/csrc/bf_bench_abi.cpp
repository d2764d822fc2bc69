// bf_bench_abi.cpp -- the measurement and test ABI of libdsabf.so: exactly what include/dsabf_bench.h declares.
#include "../../include/dsabf_bench.h"

#include <cstring>

#include "bf_runtime_internal.h"

extern "C" {

int bf_mfma_peak_device(bf_handle* h, const void* d_operands, size_t operand_bytes, void* d_scratch, size_t scratch_bytes, int iters,
                        double* ops, void* hip_stream)
{
    if (!h || !d_operands || !d_scratch) return fail(BF_ERR_INVALID, "NULL argument");
    if (operand_bytes < dsabf::kMfmaPeakSrcBytes || scratch_bytes < dsabf::kMfmaPeakSinkBytes || ((uintptr_t)d_operands & 15) || iters <= 0)
        return fail(BF_ERR_INVALID, "need >= %zu operand bytes (16-byte aligned), >= %zu scratch bytes, iters > 0",
                    dsabf::kMfmaPeakSrcBytes, dsabf::kMfmaPeakSinkBytes);
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_mfma_peak(d_operands, d_scratch, iters, h->n_cus, ops, as_stream(hip_stream)));
    return BF_OK;
}

int bf_gather_relayout_device(bf_handle* h, const float* d_stage, float* d_full, size_t rows_held, int world, size_t row_floats,
                              int skip_rank, void* hip_stream)
{
    if (!h || !d_stage || !d_full) return fail(BF_ERR_INVALID, "NULL argument");
    if (world < 1 || row_floats % 4 || ((uintptr_t)d_stage & 15) || ((uintptr_t)d_full & 15))
        return fail(BF_ERR_INVALID, "need world >= 1, row_floats a multiple of 4 and 16-byte aligned pointers");
    ON_DEVICE(h);
    HIP_TRY(dsabf::launch_gather_relayout(d_stage, d_full, rows_held, world, row_floats, skip_rank, h->n_cus, as_stream(hip_stream)));
    return BF_OK;
}

int bf_set_switch(bf_handle* h, const char* name, int value)
{
    if (!h || !name) return fail(BF_ERR_INVALID, "NULL argument");
    ON_DEVICE(h);
    if (!strcmp(name, "tsplit")) {
        if (value < 0) return fail(BF_ERR_INVALID, "tsplit must be >= 0 (0: the library decides)");
        h->geom.tsplit = value;
    } else if (!strcmp(name, "rtw_kout")) {
        if (value < 0 || value > 32) return fail(BF_ERR_INVALID, "rtw_kout must be 0 .. 32 (0: the library decides)");
        h->geom.rtw_kout = value;
    } else if (!strcmp(name, "lds_pad")) {
        if (value < 0 || value > dsabf::kLdsPerCuBytes) return fail(BF_ERR_INVALID, "lds_pad must be 0 .. %d bytes", dsabf::kLdsPerCuBytes);
        h->geom.lds_pad = value;
        // (the antenna-fold kernel's launcher asks for the default 48 KiB of dynamic LDS at most: a pad beyond that hands the handle
        //  back to the kernel the weights select otherwise -- its image is resident -- until the next bf_set_weights)
        if (h->geom.fold && dsabf::fused_launch_shape(h->geom, 1, h->n_cus).lds_bytes > 48 * 1024) {
            FLUSH_UNITS(h);
            h->geom.fold = false;
        }
    } else if (!strcmp(name, "dm_wide")) {
        h->geom.dm_wide = value != 0;
    } else if (!strcmp(name, "coalesce")) {
        FLUSH_UNITS(h);
        h->coalesce = value != 0;
    } else if (!strcmp(name, "paired")) {
        h->force_general = value == 0;   // takes effect at the next bf_set_weights (the kernel is chosen per weight set)
    } else if (!strcmp(name, "fold")) {
        h->no_fold = value == 0;         // takes effect at the next bf_set_weights, like "paired" (which, at 0, rules the fold kernel out too)
    } else if (!strcmp(name, "dm_ring")) {
        h->dm_ring = value != 0;         // takes effect at the next bf_dm_stream_create
    } else if (!strcmp(name, "cal_resident")) {
        h->cal_resident = value != 0;    // 0: bf_solve_gains_device streams the visibilities at every antenna count (same bits)
    } else if (!strcmp(name, "null_resident")) {
        h->null_resident = value != 0;   // 0: bf_null_solve_device streams the visibilities at every antenna count (same bits)
    } else {
        return fail(BF_ERR_INVALID, "unknown switch \"%s\" (tsplit, rtw_kout, lds_pad, dm_wide, dm_ring, paired, fold, coalesce, cal_resident, null_resident)", name);
    }
    return BF_OK;
}

int bf_get_counter(const bf_handle* h, const char* name, uint64_t* value)
{
    if (!h || !name || !value) return fail(BF_ERR_INVALID, "NULL argument");
    if (!strcmp(name, "fused_launches"))
        *value = h->n_fused_launches;
    else if (!strcmp(name, "queued_units"))
        *value = h->pending.size();
    else if (!strcmp(name, "dm_ring_stages")) {   // live DM stages of this handle whose buffer is the twice-mapped ring (the rest: linear)
        uint64_t n = 0;
        for (const bf_stage* s : h->stages) n += s->ring ? 1 : 0;
        *value = n;
    } else if (!strcmp(name, "fold_stream"))       // 1: the antenna-fold launch of this handle is fused16_fold_stream_kernel (whole chunk spans)
        *value = dsabf::fold_streams(h->geom) ? 1 : 0;
    else if (!strcmp(name, "dm_wide_groups") || !strcmp(name, "dm_wide_mask")) {   // the groups the shared-window kernel took in the most recent DM launch
        uint64_t groups = 0, mask = 0;
        if (int rc = dm_wide_taken(h, &groups, &mask)) return rc;
        *value = !strcmp(name, "dm_wide_groups") ? groups : mask;
    } else
        return fail(BF_ERR_INVALID, "unknown counter \"%s\" (fused_launches, queued_units, dm_ring_stages, fold_stream, dm_wide_groups, dm_wide_mask)", name);
    return BF_OK;
}

int bf_kernel_info(const bf_handle* h, int n_units, int* grid, int* block, int* lds_bytes, int* vgprs)
{
    if (!h) return fail(BF_ERR_INVALID, "handle is NULL");
    const dsabf::LaunchShape ls = dsabf::fused_launch_shape(h->geom, n_units > 0 ? n_units : 1, h->n_cus);
    if (grid) *grid = ls.grid;
    if (block) *block = ls.block;
    if (lds_bytes) *lds_bytes = ls.lds_bytes;
    if (vgprs) *vgprs = dsabf::fused_vgprs(h->geom);
    return BF_OK;
}

int bf_launch_plan(const bf_config* cfg, int paired, int n_units, int n_cus, int* grid, int* block, int* lds_bytes, char* name,
                   size_t name_len)
{
    dsabf::Geometry g{};
    if (int rc = supported_geom(cfg, g)) return rc;
    if (n_units <= 0 || n_cus <= 0) return fail(BF_ERR_INVALID, "need n_units > 0 and n_cus > 0");
    g.paired = paired && dsabf::pairing_supported(g);   // what bf_set_weights decides for a conjugate-symmetric weight set
    const dsabf::LaunchShape ls = dsabf::fused_launch_shape(g, n_units, n_cus);
    if (grid) *grid = ls.grid;
    if (block) *block = ls.block;
    if (lds_bytes) *lds_bytes = ls.lds_bytes;
    if (name && name_len) dsabf::fused_kernel_name(g, name, name_len);
    return BF_OK;
}

int bf_rtw_plan(const bf_config* cfg, int n_units, int n_cus, int* windows_per_stream, int* chunks_total)
{
    dsabf::Geometry g{};
    if (int rc = supported_geom(cfg, g)) return rc;
    if (n_units <= 0 || n_cus <= 0) return fail(BF_ERR_INVALID, "need n_units > 0 and n_cus > 0");
    const dsabf::LaunchShape ls = dsabf::fused_launch_shape(g, n_units, n_cus);
    if (windows_per_stream) *windows_per_stream = ls.rt_kout;
    if (chunks_total) *chunks_total = ls.chunks_total;
    return BF_OK;
}

int bf_kernel_name(const bf_handle* h, char* buf, size_t buflen)
{
    if (!h || !buf || !buflen) return fail(BF_ERR_INVALID, "NULL argument");
    dsabf::fused_kernel_name(h->geom, buf, buflen);
    return BF_OK;
}

int bf_variant_key(const bf_config* cfg, int paired, int write_c, char* buf, size_t buflen)
{
    if (!buf || !buflen) return fail(BF_ERR_INVALID, "NULL argument");
    dsabf::Geometry g{};
    if (int rc = supported_geom(cfg, g)) return rc;
    g.paired = paired && dsabf::pairing_supported(g);
    dsabf::fused_variant_key(g, write_c != 0, buf, buflen);
    return BF_OK;
}

int bf_handle_variant_key(const bf_handle* h, int write_c, char* buf, size_t buflen)
{
    if (!h || !buf || !buflen) return fail(BF_ERR_INVALID, "NULL argument");
    dsabf::fused_variant_key(h->geom, write_c != 0, buf, buflen);
    return BF_OK;
}

}  // extern "C"
