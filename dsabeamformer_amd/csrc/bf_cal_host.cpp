// bf_cal_host.cpp -- host mirror of the gain solver (include/dsabf_host.hpp: gains_file_sink, read_gains_layer, solve_vis_file,
// set_weights_calibrated, and the flag files that feed them: read_index_file, read_moments_sum, select_moments_file; docs/CALIBRATION.md)
// and of the spatial null (null_file_sink, read_null_vectors, null_vis_file, set_weights_conditioned; docs/NULLING.md).  The C-ABI's solver and weight calls take device pointers and the C-ABI has no device
// allocator, so this is the one host-mirror file that allocates device memory itself.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

#include "../../include/dsabf_host.hpp"
#include "bf_host_internal.h"

namespace dsabf {

namespace {

bool write_all(int fd, const char* p, size_t n)
{
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w <= 0) return false;
        p += w;
        n -= (size_t)w;
    }
    return true;
}

bool pread_all(int fd, void* dst, size_t n, off_t at)
{
    char* p = static_cast<char*>(dst);
    while (n) {
        const ssize_t r = ::pread(fd, p, n, at);
        if (r <= 0) return false;
        p += r;
        n -= (size_t)r;
        at += r;
    }
    return true;
}

struct fd_guard {
    int fd;
    ~fd_guard()
    {
        if (fd >= 0) ::close(fd);
    }
};

// device memory of one call, freed when it returns; the caller's current device is put back
struct device_scratch {
    int prev = -1;
    std::vector<void*> ptrs;
    hipError_t begin(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        return hipSetDevice(device);
    }
    template <typename T>
    hipError_t alloc(T** p, size_t bytes)
    {
        hipError_t e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) ptrs.push_back(*p);
        return e;
    }
    ~device_scratch()
    {
        for (void* p : ptrs) (void)hipFree(p);
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int hip_fail(const char* what, hipError_t e)
{
    return set_error(BF_ERR_DEVICE, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

}  // namespace

gains_file_sink::gains_file_sink(int n_ant, int pol_out, int n_freq, int first_channel, const char* path)
    : n_gain_doubles((size_t)pol_out * n_freq * n_ant * 2), n_info((size_t)pol_out * n_freq * 2)
{
    fd = ::open(path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return;
    char header[kHeaderBytes];
    ::memset(header, 0, sizeof(header));
    ::snprintf(header, sizeof(header),
               "HDR_VERSION 1.0\nHDR_SIZE %zu\nINSTRUMENT DSA\nCONTENT gains\nDTYPE float64\nENDIAN little\nLAYOUT pol,freq,ant,reim\n"
               "RECORD_HEADER_BYTES %zu\nNANT %d\nNPOL %d\nNFREQ %d\nFIRST_CHANNEL %d\nINFO int32 pol,freq,(iterations,status)\n",
               kHeaderBytes, kRecordBytes, n_ant, pol_out, n_freq, first_channel);
    if (!write_all(fd, header, sizeof(header))) close();
}

gains_file_sink::~gains_file_sink() { close(); }

bool gains_file_sink::deliver(uint64_t first_block, uint64_t n_columns_per_pol, const double* gains, const int32_t* info)
{
    if (fd < 0) return false;
    const uint64_t rec[2] = {first_block, n_columns_per_pol};
    static_assert(sizeof rec == kRecordBytes, "the record header is two uint64");
    if (!write_all(fd, reinterpret_cast<const char*>(rec), sizeof rec) ||
        !write_all(fd, reinterpret_cast<const char*>(gains), n_gain_doubles * sizeof(double)) ||
        !write_all(fd, reinterpret_cast<const char*>(info), n_info * sizeof(int32_t)))
        return false;
    records++;
    return true;
}

void gains_file_sink::close()
{
    if (fd >= 0) ::close(fd);
    fd = -1;
}

bool read_record_file_header(const char* path, record_file_header* out, std::string* why)
{
    auto no = [&](const std::string& msg) {
        if (why) *why = std::string(path) + ": " + msg;
        return false;
    };
    fd_guard f{::open(path, O_RDONLY)};
    if (f.fd < 0) return no("cannot be opened");
    struct stat st;
    char text[4097];
    if (::fstat(f.fd, &st) != 0 || st.st_size < 4096 || !pread_all(f.fd, text, 4096, 0)) return no("is shorter than its 4096-byte header");
    text[4096] = 0;
    std::map<std::string, std::string> kv;
    std::istringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        const size_t sp = line.find(' ');
        if (sp != std::string::npos) kv[line.substr(0, sp)] = line.substr(sp + 1);
    }
    for (const char* key : {"HDR_SIZE", "CONTENT", "DTYPE", "RECORD_HEADER_BYTES", "NANT", "NPOL", "NFREQ", "FIRST_CHANNEL"})
        if (!kv.count(key)) return no(std::string("its header has no ") + key);
    record_file_header h;
    h.content = kv["CONTENT"];
    h.dtype = kv["DTYPE"];
    h.n_ant = atoi(kv["NANT"].c_str());
    h.n_pol = atoi(kv["NPOL"].c_str());
    h.n_freq = atoi(kv["NFREQ"].c_str());
    h.first_channel = atoi(kv["FIRST_CHANNEL"].c_str());
    h.header_bytes = (size_t)atoll(kv["HDR_SIZE"].c_str());
    h.record_header_bytes = (size_t)atoll(kv["RECORD_HEADER_BYTES"].c_str());
    h.file_bytes = (size_t)st.st_size;
    if (h.n_ant <= 0 || h.n_pol <= 0 || h.n_freq <= 0 || h.first_channel < 0 || h.header_bytes != 4096 || h.record_header_bytes != 16)
        return no("its header does not describe a record file of this library");
    *out = h;
    return true;
}

bool read_gains_layer(const char* path, int n_ant, int n_freq, int first_channel, std::vector<double>* layer, std::string* why)
{
    record_file_header h;
    if (!read_record_file_header(path, &h, why)) return false;
    auto no = [&](const std::string& msg) {
        if (why) *why = std::string(path) + ": " + msg;
        return false;
    };
    if (h.content != "gains" || h.dtype != "float64") return no("CONTENT " + h.content + " is not a file of gains");
    if (h.n_ant != n_ant || h.n_freq != n_freq || h.first_channel != first_channel)
        return no("NANT " + std::to_string(h.n_ant) + " NFREQ " + std::to_string(h.n_freq) + " FIRST_CHANNEL " + std::to_string(h.first_channel) +
                  " do not match this run (" + std::to_string(n_ant) + " antennas, " + std::to_string(n_freq) + " channels from " +
                  std::to_string(first_channel) + ")");
    const size_t layer_bytes = (size_t)n_freq * n_ant * 2 * sizeof(double);
    const size_t rec_bytes = h.record_header_bytes + (size_t)h.n_pol * layer_bytes + (size_t)h.n_pol * n_freq * 2 * sizeof(int32_t);
    const size_t body = h.file_bytes - h.header_bytes;
    if (body == 0 || body % rec_bytes) return no("holds no whole record");
    fd_guard f{::open(path, O_RDONLY)};
    layer->resize((size_t)n_freq * n_ant * 2);
    if (f.fd < 0 || !pread_all(f.fd, layer->data(), layer_bytes, (off_t)(h.header_bytes + body - rec_bytes + h.record_header_bytes)))
        return no("its last record cannot be read");
    return true;
}

int solve_vis_file(const char* vis_path, const char* gains_path, bool joint_pol, int device, uint64_t* n_records, std::ostream& log,
                   const uint8_t* ant_flags)
{
    record_file_header vh;
    std::string why;
    if (!read_record_file_header(vis_path, &vh, &why)) return set_error(BF_ERR_INVALID, why.c_str());
    if (vh.content != "visibilities" || vh.dtype != "int64") return set_error(BF_ERR_INVALID, (std::string(vis_path) + " is not a file of visibilities").c_str());
    bf_config cfg;
    bf_config_default(&cfg, /*debug=*/0);   // the solver reads n_ant, n_pol and n_freq of the handle's geometry only
    cfg.n_ant = vh.n_ant;
    cfg.n_pol = vh.n_pol;
    cfg.n_freq = vh.n_freq;
    const int pol_out = joint_pol ? 1 : cfg.n_pol;
    const size_t n_vis = 2 * bf_corr_entries(&cfg), n_gains = 2 * bf_cal_gain_entries(&cfg, joint_pol), n_info = (size_t)pol_out * cfg.n_freq * 2;
    const size_t rec_bytes = vh.record_header_bytes + n_vis * sizeof(int64_t), body = vh.file_bytes - vh.header_bytes;
    if (body % rec_bytes) return set_error(BF_ERR_INVALID, (std::string(vis_path) + " ends inside a record").c_str());
    fd_guard in{::open(vis_path, O_RDONLY)};
    if (in.fd < 0) return set_error(BF_ERR_INVALID, (std::string(vis_path) + " cannot be opened").c_str());
    bf_handle* h = nullptr;
    int rc = bf_create(&cfg, device, &h);
    if (rc != BF_OK) return rc;
    struct handle_guard {
        bf_handle* h;
        ~handle_guard() { bf_destroy(h); }
    } hg{h};
    gains_file_sink sink(cfg.n_ant, pol_out, cfg.n_freq, vh.first_channel, gains_path);
    if (!sink.is_open()) return set_error(BF_ERR_INVALID, (std::string(gains_path) + " cannot be created").c_str());
    device_scratch mem;
    hipError_t e = mem.begin(device);
    int64_t* d_vis = nullptr;
    double* d_gains = nullptr;
    int32_t* d_info = nullptr;
    uint8_t* d_flags = nullptr;
    if (e == hipSuccess && ant_flags) e = mem.alloc(&d_flags, (size_t)cfg.n_ant);
    if (e == hipSuccess && ant_flags) e = hipMemcpy(d_flags, ant_flags, (size_t)cfg.n_ant, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mem.alloc(&d_vis, n_vis * sizeof(int64_t));
    if (e == hipSuccess) e = mem.alloc(&d_gains, n_gains * sizeof(double));
    if (e == hipSuccess) e = mem.alloc(&d_info, n_info * sizeof(int32_t));
    if (e != hipSuccess) return hip_fail("solve_vis_file", e);
    std::vector<int64_t> vis(n_vis);
    std::vector<double> gains(n_gains);
    std::vector<int32_t> info(n_info);
    bf_cal_options opt;
    bf_cal_default_options(&opt);
    opt.joint_pol = joint_pol ? 1 : 0;
    uint64_t converged = 0, problems = 0;
    for (size_t at = vh.header_bytes; at < vh.file_bytes; at += rec_bytes) {
        uint64_t rec[2];
        if (!pread_all(in.fd, rec, sizeof rec, (off_t)at) || !pread_all(in.fd, vis.data(), n_vis * sizeof(int64_t), (off_t)(at + sizeof rec)))
            return set_error(BF_ERR_INVALID, (std::string(vis_path) + ": a record cannot be read").c_str());
        if ((e = hipMemcpy(d_vis, vis.data(), n_vis * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) return hip_fail("solve_vis_file", e);
        if ((rc = solve_gains(h, d_vis, nullptr, d_flags, opt, d_gains, d_info)) != BF_OK) return rc;
        if ((e = hipMemcpy(gains.data(), d_gains, n_gains * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("solve_vis_file", e);
        if ((e = hipMemcpy(info.data(), d_info, n_info * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("solve_vis_file", e);
        if (!sink.deliver(rec[0], rec[1], gains.data(), info.data())) return set_error(BF_ERR_INVALID, (std::string(gains_path) + ": write failed").c_str());
        for (size_t i = 0; i < n_info; i += 2, problems++) converged += info[i + 1] == 1;
    }
    if (n_records) *n_records = sink.get_records_written();
    log << "Gain solver: " << sink.get_records_written() << " records of " << pol_out << " x " << cfg.n_freq << " problems (" << cfg.n_ant << " antennas), "
        << converged << " of " << problems << " converged" << std::endl;
    return BF_OK;
}

bool read_index_file(const char* path, int n, std::vector<uint8_t>* flags, std::string* why)
{
    auto no = [&](const std::string& msg) {
        if (why) *why = std::string(path) + ": " + msg;
        return false;
    };
    std::ifstream in(path);
    if (!in) return no("could not be read");
    flags->assign((size_t)n, 0);
    std::string line;
    while (std::getline(in, line)) {
        line = line.substr(0, line.find('#'));
        const size_t a = line.find_first_not_of(" \t\r");
        if (a == std::string::npos) continue;
        char* end = nullptr;
        const long i = strtol(line.c_str() + a, &end, 10);
        while (*end == ' ' || *end == '\t' || *end == '\r') end++;
        if (end == line.c_str() + a || *end || i < 0 || i >= n) return no("'" + line.substr(a) + "' is not an index 0 .. " + std::to_string(n - 1));
        (*flags)[(size_t)i] = 1;
    }
    return true;
}

bool read_moments_sum(const char* path, record_file_header* header, std::vector<int64_t>* moments, uint64_t* n_columns_per_pol, std::string* why)
{
    record_file_header h;
    if (!read_record_file_header(path, &h, why)) return false;
    auto no = [&](const std::string& msg) {
        if (why) *why = std::string(path) + ": " + msg;
        return false;
    };
    if (h.content != "voltage_moments" || h.dtype != "int64") return no("CONTENT " + h.content + " is not a file of voltage moments");
    const size_t n = (size_t)h.n_freq * h.n_pol * h.n_ant * 2;
    const size_t rec_bytes = h.record_header_bytes + n * sizeof(int64_t), body = h.file_bytes - h.header_bytes;
    if (body == 0 || body % rec_bytes) return no("holds no whole record");
    fd_guard f{::open(path, O_RDONLY)};
    if (f.fd < 0) return no("cannot be opened");
    moments->assign(n, 0);
    std::vector<int64_t> one(n);
    uint64_t columns = 0;
    for (size_t at = h.header_bytes; at < h.file_bytes; at += rec_bytes) {
        uint64_t rec[2];
        if (!pread_all(f.fd, rec, sizeof rec, (off_t)at) || !pread_all(f.fd, one.data(), n * sizeof(int64_t), (off_t)(at + sizeof rec)))
            return no("a record cannot be read");
        for (size_t i = 0; i < n; i++) (*moments)[i] += one[i];
        columns += rec[1];
    }
    *header = h;
    *n_columns_per_pol = columns;
    return true;
}

int select_moments_file(const char* moments_path, const bf_sk_options& opt, const char* ant_path, const char* chan_path, std::ostream& log)
{
    record_file_header h;
    std::vector<int64_t> moments;
    uint64_t columns = 0;
    std::string why;
    if (!read_moments_sum(moments_path, &h, &moments, &columns, &why)) return set_error(BF_ERR_INVALID, why.c_str());
    std::vector<uint8_t> ant((size_t)h.n_ant), chan((size_t)h.n_freq);
    const int rc = bf_sk_select(moments.data(), columns, h.n_freq, h.n_pol, h.n_ant, &opt, nullptr, nullptr, ant.data(), chan.data());
    if (rc != BF_OK) return rc;
    auto write = [&](const char* path, const char* what, const std::vector<uint8_t>& flags, int offset) {
        std::ofstream out(path);
        out << "# " << what << " flagged by spectral kurtosis (beam -e " << moments_path << "): " << columns << " columns per polarisation, centre "
            << opt.centre << ", " << opt.n_sigma << " sigma\n";
        for (size_t i = 0; i < flags.size(); i++)
            if (flags[i]) out << (long)i + offset << "\n";
        out.close();
        return !out.fail();
    };
    if (!write(ant_path, "antennas", ant, 0)) return set_error(BF_ERR_INVALID, (std::string(ant_path) + " cannot be written").c_str());
    if (chan_path && !write(chan_path, "channels", chan, h.first_channel)) return set_error(BF_ERR_INVALID, (std::string(chan_path) + " cannot be written").c_str());
    size_t n_ant = 0, n_chan = 0;
    for (uint8_t f : ant) n_ant += f != 0;
    for (uint8_t f : chan) n_chan += f != 0;
    log << "Spectral kurtosis: " << columns << " columns per polarisation, " << n_ant << " of " << h.n_ant << " antennas and " << n_chan << " of "
        << h.n_freq << " channels flagged" << std::endl;
    return BF_OK;
}

int set_weights_calibrated(bf_handle* h, int device, const int8_t* w, const double* gains_layer, int8_t* w_set, const uint8_t* ant_flags)
{
    if (!gains_layer) return set_error(BF_ERR_INVALID, "set_weights_calibrated: NULL argument");
    return set_weights_conditioned(h, device, w, gains_layer, nullptr, w_set, ant_flags);
}

int set_weights_conditioned(bf_handle* h, int device, const int8_t* w, const double* gains_layer, const null_vectors* nulls, int8_t* w_set,
                            const uint8_t* ant_flags)
{
    if (!h || !w || (!gains_layer && !nulls)) return set_error(BF_ERR_INVALID, "set_weights_conditioned: NULL argument");
    bf_config cfg;
    int rc = bf_get_config(h, &cfg);
    if (rc != BF_OK) return rc;
    const size_t w_bytes = (size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2, g_bytes = (size_t)cfg.n_freq * cfg.n_ant * 2 * sizeof(double);
    device_scratch mem;
    hipError_t e = mem.begin(device);
    int8_t* d_w = nullptr;
    double *d_g = nullptr, *d_vecs = nullptr;
    int32_t* d_info = nullptr;
    uint8_t* d_flags = nullptr;
    if (nulls && (nulls->n_null < 1 || nulls->n_null > BF_NULL_MAX || nulls->vecs.size() != (size_t)cfg.n_freq * nulls->n_null * cfg.n_ant * 2 ||
                  nulls->info.size() != (size_t)cfg.n_freq * (1 + 2 * nulls->n_null)))
        return set_error(BF_ERR_INVALID, "set_weights_conditioned: the vectors are not of this geometry");
    if (e == hipSuccess && ant_flags) e = mem.alloc(&d_flags, (size_t)cfg.n_ant);
    if (e == hipSuccess && ant_flags) e = hipMemcpy(d_flags, ant_flags, (size_t)cfg.n_ant, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mem.alloc(&d_w, w_bytes);
    if (e == hipSuccess) e = hipMemcpy(d_w, w, w_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && gains_layer) e = mem.alloc(&d_g, g_bytes);
    if (e == hipSuccess && gains_layer) e = hipMemcpy(d_g, gains_layer, g_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && nulls) e = mem.alloc(&d_vecs, nulls->vecs.size() * sizeof(double));
    if (e == hipSuccess && nulls) e = hipMemcpy(d_vecs, nulls->vecs.data(), nulls->vecs.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && nulls) e = mem.alloc(&d_info, nulls->info.size() * sizeof(int32_t));
    if (e == hipSuccess && nulls) e = hipMemcpy(d_info, nulls->info.data(), nulls->info.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("set_weights_conditioned", e);
    // (in place, on the null stream: the calibration first, then the null)
    if (gains_layer && (rc = calibrate_weights(h, d_w, d_g, d_flags, BF_CAL_PHASE, d_w)) != BF_OK) return rc;
    if (nulls && (rc = null_weights(h, d_w, d_vecs, d_info, nulls->n_null, d_flags, BF_NULL_SCALED, d_w)) != BF_OK) return rc;
    if ((rc = bf_set_weights_device(h, d_w, nullptr)) != BF_OK) return rc;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail("set_weights_conditioned", e);    // d_w is freed on return
    if (w_set && (e = hipMemcpy(w_set, d_w, w_bytes, hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("set_weights_conditioned", e);
    return BF_OK;
}

// ---- the spatial null (docs/NULLING.md) ------------------------------------------------------------------------------------------

null_file_sink::null_file_sink(int n_ant, int n_freq, int first_channel, int n_null, const char* path)
    : n_vec_doubles((size_t)n_freq * n_null * n_ant * 2), n_eig((size_t)n_freq * (n_null + 1)), n_info((size_t)n_freq * (1 + 2 * n_null))
{
    fd = ::open(path, O_CREAT | O_TRUNC | O_WRONLY, 0644);
    if (fd < 0) return;
    char header[kHeaderBytes];
    ::memset(header, 0, sizeof(header));
    ::snprintf(header, sizeof(header),
               "HDR_VERSION 1.0\nHDR_SIZE %zu\nINSTRUMENT DSA\nCONTENT nullvecs\nDTYPE float64\nENDIAN little\nLAYOUT freq,vec,ant,reim\n"
               "RECORD_HEADER_BYTES %zu\nNANT %d\nNPOL 1\nNFREQ %d\nFIRST_CHANNEL %d\nNNULL %d\nEIG float64 freq,(lambdas,trace)\n"
               "INFO int32 freq,(n_used,(iterations,status) per vector)\n",
               kHeaderBytes, kRecordBytes, n_ant, n_freq, first_channel, n_null);
    if (!write_all(fd, header, sizeof(header))) close();
}

null_file_sink::~null_file_sink() { close(); }

bool null_file_sink::deliver(uint64_t first_block, uint64_t n_columns_per_pol, const double* vecs, const double* eig, const int32_t* info)
{
    if (fd < 0) return false;
    const uint64_t rec[2] = {first_block, n_columns_per_pol};
    static_assert(sizeof rec == kRecordBytes, "the record header is two uint64");
    if (!write_all(fd, reinterpret_cast<const char*>(rec), sizeof rec) ||
        !write_all(fd, reinterpret_cast<const char*>(vecs), n_vec_doubles * sizeof(double)) ||
        !write_all(fd, reinterpret_cast<const char*>(eig), n_eig * sizeof(double)) ||
        !write_all(fd, reinterpret_cast<const char*>(info), n_info * sizeof(int32_t)))
        return false;
    records++;
    return true;
}

void null_file_sink::close()
{
    if (fd >= 0) ::close(fd);
    fd = -1;
}

bool read_null_vectors(const char* path, int n_ant, int n_freq, int first_channel, null_vectors* out, std::string* why)
{
    record_file_header h;
    if (!read_record_file_header(path, &h, why)) return false;
    auto no = [&](const std::string& msg) {
        if (why) *why = std::string(path) + ": " + msg;
        return false;
    };
    if (h.content != "nullvecs" || h.dtype != "float64") return no("CONTENT " + h.content + " is not a file of interferer vectors");
    if (h.n_ant != n_ant || h.n_freq != n_freq || h.first_channel != first_channel)
        return no("NANT " + std::to_string(h.n_ant) + " NFREQ " + std::to_string(h.n_freq) + " FIRST_CHANNEL " + std::to_string(h.first_channel) +
                  " do not match this run (" + std::to_string(n_ant) + " antennas, " + std::to_string(n_freq) + " channels from " +
                  std::to_string(first_channel) + ")");
    fd_guard f{::open(path, O_RDONLY)};
    char text[4097];
    if (f.fd < 0 || !pread_all(f.fd, text, 4096, 0)) return no("cannot be read");
    text[4096] = 0;
    const char* key = ::strstr(text, "\nNNULL ");
    const int n_null = key ? atoi(key + 7) : 0;
    if (n_null < 1 || n_null > BF_NULL_MAX) return no("its header has no NNULL 1 .. " + std::to_string(BF_NULL_MAX));
    const size_t vec_bytes = (size_t)n_freq * n_null * n_ant * 2 * sizeof(double), eig_bytes = (size_t)n_freq * (n_null + 1) * sizeof(double);
    const size_t info_bytes = (size_t)n_freq * (1 + 2 * n_null) * sizeof(int32_t);
    const size_t rec_bytes = h.record_header_bytes + vec_bytes + eig_bytes + info_bytes, body = h.file_bytes - h.header_bytes;
    if (body == 0 || body % rec_bytes) return no("holds no whole record");
    const off_t last = (off_t)(h.header_bytes + body - rec_bytes + h.record_header_bytes);
    out->n_null = n_null;
    out->vecs.resize(vec_bytes / sizeof(double));
    out->info.resize(info_bytes / sizeof(int32_t));
    if (!pread_all(f.fd, out->vecs.data(), vec_bytes, last) || !pread_all(f.fd, out->info.data(), info_bytes, last + (off_t)(vec_bytes + eig_bytes)))
        return no("its last record cannot be read");
    return true;
}

int null_vis_file(const char* vis_path, const char* null_path, const bf_null_options& opt, int device, uint64_t* n_records, std::ostream& log,
                  const uint8_t* ant_flags)
{
    record_file_header vh;
    std::string why;
    if (!read_record_file_header(vis_path, &vh, &why)) return set_error(BF_ERR_INVALID, why.c_str());
    if (vh.content != "visibilities" || vh.dtype != "int64") return set_error(BF_ERR_INVALID, (std::string(vis_path) + " is not a file of visibilities").c_str());
    bf_config cfg;
    bf_config_default(&cfg, /*debug=*/0);   // the solver reads n_ant, n_pol and n_freq of the handle's geometry only
    cfg.n_ant = vh.n_ant;
    cfg.n_pol = vh.n_pol;
    cfg.n_freq = vh.n_freq;
    const size_t n_vis = 2 * bf_corr_entries(&cfg), n_vecs = 2 * bf_null_vec_entries(&cfg, opt.n_null);
    if (!n_vecs) return set_error(BF_ERR_INVALID, "null_vis_file: n_null is outside 1 ... 4");
    const size_t n_eig = (size_t)cfg.n_freq * (opt.n_null + 1), n_info = (size_t)cfg.n_freq * (1 + 2 * opt.n_null);
    const size_t rec_bytes = vh.record_header_bytes + n_vis * sizeof(int64_t), body = vh.file_bytes - vh.header_bytes;
    if (body % rec_bytes) return set_error(BF_ERR_INVALID, (std::string(vis_path) + " ends inside a record").c_str());
    fd_guard in{::open(vis_path, O_RDONLY)};
    if (in.fd < 0) return set_error(BF_ERR_INVALID, (std::string(vis_path) + " cannot be opened").c_str());
    bf_handle* h = nullptr;
    int rc = bf_create(&cfg, device, &h);
    if (rc != BF_OK) return rc;
    struct handle_guard {
        bf_handle* h;
        ~handle_guard() { bf_destroy(h); }
    } hg{h};
    null_file_sink sink(cfg.n_ant, cfg.n_freq, vh.first_channel, opt.n_null, null_path);
    if (!sink.is_open()) return set_error(BF_ERR_INVALID, (std::string(null_path) + " cannot be created").c_str());
    device_scratch mem;
    hipError_t e = mem.begin(device);
    int64_t* d_vis = nullptr;
    double *d_vecs = nullptr, *d_eig = nullptr;
    int32_t* d_info = nullptr;
    uint8_t* d_flags = nullptr;
    if (e == hipSuccess && ant_flags) e = mem.alloc(&d_flags, (size_t)cfg.n_ant);
    if (e == hipSuccess && ant_flags) e = hipMemcpy(d_flags, ant_flags, (size_t)cfg.n_ant, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mem.alloc(&d_vis, n_vis * sizeof(int64_t));
    if (e == hipSuccess) e = mem.alloc(&d_vecs, n_vecs * sizeof(double));
    if (e == hipSuccess) e = mem.alloc(&d_eig, n_eig * sizeof(double));
    if (e == hipSuccess) e = mem.alloc(&d_info, n_info * sizeof(int32_t));
    if (e != hipSuccess) return hip_fail("null_vis_file", e);
    std::vector<int64_t> vis(n_vis);
    std::vector<double> vecs(n_vecs), eig(n_eig);
    std::vector<int32_t> info(n_info);
    uint64_t used = 0, channels = 0;
    for (size_t at = vh.header_bytes; at < vh.file_bytes; at += rec_bytes) {
        uint64_t rec[2];
        if (!pread_all(in.fd, rec, sizeof rec, (off_t)at) || !pread_all(in.fd, vis.data(), n_vis * sizeof(int64_t), (off_t)(at + sizeof rec)))
            return set_error(BF_ERR_INVALID, (std::string(vis_path) + ": a record cannot be read").c_str());
        if ((e = hipMemcpy(d_vis, vis.data(), n_vis * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess) return hip_fail("null_vis_file", e);
        if ((rc = null_solve(h, d_vis, d_flags, opt, d_vecs, d_eig, d_info)) != BF_OK) return rc;
        if ((e = hipMemcpy(vecs.data(), d_vecs, n_vecs * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("null_vis_file", e);
        if ((e = hipMemcpy(eig.data(), d_eig, n_eig * sizeof(double), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("null_vis_file", e);
        if ((e = hipMemcpy(info.data(), d_info, n_info * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("null_vis_file", e);
        if (!sink.deliver(rec[0], rec[1], vecs.data(), eig.data(), info.data()))
            return set_error(BF_ERR_INVALID, (std::string(null_path) + ": write failed").c_str());
        for (size_t i = 0; i < n_info; i += 1 + 2 * (size_t)opt.n_null, channels++) used += (uint64_t)info[i];
    }
    if (n_records) *n_records = sink.get_records_written();
    log << "Spatial null: " << sink.get_records_written() << " records of " << cfg.n_freq << " channels (" << cfg.n_ant << " antennas, up to " << opt.n_null
        << " vectors each), " << used << " vectors used in " << channels << " channel solves" << std::endl;
    return BF_OK;
}

}  // namespace dsabf
