// bf_rm_host.cpp -- host mirror of Faraday synthesis (include/dsabf_host.hpp: faraday_options, read_coherent_header,
// faraday_coherent_file; docs/FARADAY.md section 5): `beam --faraday` -- every record of a --coherent file through bf_rm_device,
// into a file of rotation-measure spectra, fits and peak records.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <sstream>

#include "../../include/dsabf_host.hpp"
#include "bf_host_internal.h"

namespace dsabf {

namespace {

struct file_guard {
    FILE* fp;
    ~file_guard()
    {
        if (fp) fclose(fp);
    }
};

// device memory of one call, freed when it returns; the caller's current device is put back (as in bf_cdd_host.cpp)
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

int hip_fail(const char* what, hipError_t e) { return set_error(BF_ERR_DEVICE, (std::string(what) + ": " + hipGetErrorString(e)).c_str()); }

// the output file: removed again unless the whole run went through, so that a failure leaves no header-only or partial file
struct output_guard {
    const char* path;
    FILE* fp;
    bool keep = false;
    ~output_guard()
    {
        if (fp) fclose(fp);
        if (fp && !keep) remove(path);
    }
};

struct stage_guard {
    bf_handle* h = nullptr;
    bf_rm* s = nullptr;
    ~stage_guard()
    {
        if (s) bf_rm_destroy(s);
        if (h) bf_destroy(h);
    }
};

}  // namespace

bool read_coherent_header(const char* path, coherent_file_header* out, std::string* why)
{
    file_guard f{fopen(path, "rb")};
    char text[coherent_file_header_bytes + 1] = {0};
    if (!f.fp || fread(text, 1, coherent_file_header_bytes, f.fp) != coherent_file_header_bytes) {
        *why = std::string(path) + ": cannot read a " + std::to_string(coherent_file_header_bytes) + "-byte header";
        return false;
    }
    std::map<std::string, std::string> kv;
    std::istringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        const size_t sp = line.find(' ');
        if (sp != std::string::npos) kv[line.substr(0, sp)] = line.substr(sp + 1);
    }
    auto num = [&kv](const char* key) { return kv.count(key) ? atoi(kv[key].c_str()) : -1; };
    *out = coherent_file_header();
    out->n_freq = num("NFREQ"), out->first_channel = num("FIRST_CHANNEL"), out->n_time = num("NTIME"), out->n_int = num("NINT");
    out->n_avg = kv.count("NAVG") ? num("NAVG") : 1;
    if (kv["CONTENT"] != "coherent_stokes" || kv["DTYPE"] != "float32" || kv["LAYOUT"] != "time,freq,iquv" || num("HDR_SIZE") != (int)coherent_file_header_bytes ||
        num("RECORD_HEADER_BYTES") != (int)coherent_record_header_bytes || out->n_freq < 1 || out->n_freq > 4096 || out->first_channel < 0 || out->n_time < 1 ||
        out->n_int < 1 || out->n_time % out->n_int || out->n_avg < 1) {
        *why = std::string(path) + " is not a file of coherently dedispersed Stokes parameters (beam --coherent)";
        return false;
    }
    out->n_rows = (size_t)(out->n_time / out->n_int);
    fseek(f.fp, 0, SEEK_END);
    const long size = ftell(f.fp);
    const size_t record = coherent_record_header_bytes + out->n_rows * out->n_freq * 4 * sizeof(float);
    out->n_records = size < 0 ? 0 : ((size_t)size - coherent_file_header_bytes) / record;
    if (size < 0 || ((size_t)size - coherent_file_header_bytes) % record) {
        *why = std::string(path) + " does not end with a whole record of " + std::to_string(record) + " bytes";
        return false;
    }
    return true;
}

int faraday_coherent_file(const faraday_options& o, uint64_t* n_written, uint64_t* n_left_out, std::ostream& log)
{
    *n_written = *n_left_out = 0;
    coherent_file_header ch;
    std::string why;
    if (!read_coherent_header(o.coherent_path, &ch, &why)) return set_error(BF_ERR_INVALID, why.c_str());
    const int n_chan = ch.n_freq, n_rows = (int)ch.n_rows;
    std::vector<double> freq((size_t)n_chan), w((size_t)n_chan, 1.0);
    for (int c = 0; c < n_chan; c++) {
        freq[(size_t)c] = (double)channel_frequency_weights(o.gpu, ch.first_channel + c);
        if (o.chan_mask && ch.first_channel + c < o.n_mask && o.chan_mask[ch.first_channel + c]) w[(size_t)c] = 0.0;
    }
    double fwhm = 0.0, phi_max = 0.0;
    int rc = bf_rm_resolution(freq.data(), w.data(), n_chan, &fwhm, &phi_max);
    if (rc != BF_OK) return rc;
    int n_phi = o.n_phi;
    double phi0 = o.phi_lo, dphi = o.n_phi > 1 ? (o.phi_hi - o.phi_lo) / (o.n_phi - 1) : 0.0;
    if (n_phi == 0) {
        dphi = fwhm / 8.0;
        const double half = std::ceil(phi_max / dphi);
        n_phi = half >= 2047.5 ? 4096 : 2 * (int)half + 1;
        phi0 = -0.5 * (n_phi - 1) * dphi;
    }
    std::vector<float> rot((size_t)n_phi * n_chan * 2), wn((size_t)n_chan);
    double l0 = 0.0;
    if ((rc = bf_rm_table(freq.data(), w.data(), n_chan, phi0, dphi, n_phi, rot.data(), wn.data(), &l0)) != BF_OK) return rc;

    device_scratch mem;
    stage_guard g;
    hipError_t e = mem.begin(o.device);
    if (e != hipSuccess) return hip_fail("faraday_coherent_file", e);
    bf_config cfg;
    bf_config_default(&cfg, /*debug=*/1);   // (the stage takes nothing from the handle's geometry)
    if ((rc = bf_create(&cfg, o.device, &g.h)) != BF_OK) return rc;
    if ((rc = bf_rm_create(g.h, n_chan, n_phi, rot.data(), wn.data(), &g.s)) != BF_OK) return rc;

    const size_t row_floats = (size_t)n_chan * 4, n_cells = (size_t)n_rows * row_floats, n_all = (size_t)n_rows + 1;
    float *d_s = nullptr, *d_base = nullptr, *d_spec = nullptr;
    bf_rm_peak* d_peaks = nullptr;
    if ((e = mem.alloc(&d_s, (n_cells + row_floats) * sizeof(float))) != hipSuccess || (e = mem.alloc(&d_base, row_floats * sizeof(float))) != hipSuccess ||
        (e = mem.alloc(&d_spec, n_all * n_phi * 2 * sizeof(float))) != hipSuccess || (e = mem.alloc(&d_peaks, n_all * sizeof(bf_rm_peak))) != hipSuccess)
        return hip_fail("faraday_coherent_file", e);

    file_guard in{fopen(o.coherent_path, "rb")};
    output_guard out{o.out_path, in.fp ? fopen(o.out_path, "wb") : nullptr};
    if (!in.fp || !out.fp) return set_error(BF_ERR_INVALID, (std::string("cannot open ") + (in.fp ? o.out_path : o.coherent_path)).c_str());
    char header[faraday_file_header_bytes] = {0};
    snprintf(header, sizeof header,
             "HDR_SIZE %zu\nCONTENT faraday\nDTYPE float32\nNFREQ %d\nFIRST_CHANNEL %d\nNROWS %d\nNPHI %d\nPHI0 %.17g\nDPHI %.17g\nLAMBDA0_2 %.17g\nFWHM %.17g\n"
             "PHI_MAX %.17g\nRECORD_HEADER_BYTES %zu\n",
             faraday_file_header_bytes, n_chan, ch.first_channel, n_rows, n_phi, phi0, dphi, l0, fwhm, phi_max, faraday_record_header_bytes);
    if (fwrite(header, 1, sizeof header, out.fp) != sizeof header) return set_error(BF_ERR_INVALID, (std::string("cannot write ") + o.out_path).c_str());
    fseek(in.fp, (long)coherent_file_header_bytes, SEEK_SET);

    std::vector<float> cells(n_cells + row_floats), base(row_floats), spec((size_t)n_phi * 2);
    std::vector<bf_rm_peak> peaks(n_all);
    std::vector<double> series((size_t)n_rows), sum(row_floats);
    char rec_head[coherent_record_header_bytes];
    for (size_t r = 0; r < ch.n_records; r++) {
        float* rows = cells.data() + row_floats;   // (row 0 of the launch is the window's mean)
        if (fread(rec_head, 1, sizeof rec_head, in.fp) != sizeof rec_head || fread(rows, sizeof(float), n_cells, in.fp) != n_cells)
            return set_error(BF_ERR_INVALID, (std::string(o.coherent_path) + ": short record").c_str());
        int32_t width;
        memcpy(&width, rec_head + 16, 4);
        long long wl = o.window > 0 ? o.window : (long long)width * ch.n_avg / ch.n_int;
        const int win = wl < 1 ? 1 : wl > n_rows ? n_rows : (int)wl;
        for (int t = 0; t < n_rows; t++) {
            double s = 0.0;
            for (int c = 0; c < n_chan; c++) s += (double)rows[(size_t)t * row_floats + (size_t)c * 4];
            series[(size_t)t] = s;
        }
        int lo = 0;
        double best = 0.0;
        for (int t = 0; t + win <= n_rows; t++) {
            double s = series[(size_t)t];
            for (int j = 1; j < win; j++) s += series[(size_t)(t + j)];
            if (t == 0 || s > best) best = s, lo = t;
        }
        const int off_lo = lo - win, off_hi = lo + 2 * win;   // the baseline's rows: t < off_lo or t >= off_hi
        const int n_off = (off_lo > 0 ? off_lo : 0) + (off_hi < n_rows ? n_rows - off_hi : 0);
        if (n_off < faraday_min_baseline_rows) {
            (*n_left_out)++;
            continue;
        }
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int t = 0; t < n_rows; t++)
            if (t < off_lo || t >= off_hi)
                for (size_t i = 0; i < row_floats; i++) sum[i] += (double)rows[(size_t)t * row_floats + i];
        for (size_t i = 0; i < row_floats; i++) base[i] = (float)(sum[i] / n_off);
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int t = lo; t < lo + win; t++)
            for (size_t i = 0; i < row_floats; i++) sum[i] += (double)rows[(size_t)t * row_floats + i];
        for (size_t i = 0; i < row_floats; i++) cells[i] = (float)(sum[i] / win);

        if ((e = hipMemcpy(d_s, cells.data(), cells.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy(d_base, base.data(), base.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
            return hip_fail("faraday_coherent_file", e);
        if ((rc = bf_rm_device(g.s, d_s, 1, (int64_t)n_all, d_base, d_spec, d_peaks, nullptr)) != BF_OK) return rc;
        if ((e = hipMemcpy(spec.data(), d_spec, spec.size() * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = hipMemcpy(peaks.data(), d_peaks, peaks.size() * sizeof(bf_rm_peak), hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail("faraday_coherent_file", e);
        bf_rm_fit fit;
        if ((rc = bf_rm_refine(peaks.data(), 1, phi0, dphi, n_phi, l0, &fit)) != BF_OK) return rc;
        const int32_t window[2] = {lo, win};
        const double fits[4] = {fit.rm, fit.pa, fit.lin, fit.frac};
        if (fwrite(rec_head, 1, sizeof rec_head, out.fp) != sizeof rec_head || fwrite(window, 4, 2, out.fp) != 2 || fwrite(fits, 8, 4, out.fp) != 4 ||
            fwrite(spec.data(), sizeof(float), spec.size(), out.fp) != spec.size() || fwrite(peaks.data(), sizeof(bf_rm_peak), peaks.size(), out.fp) != peaks.size())
            return set_error(BF_ERR_INVALID, (std::string("cannot write ") + o.out_path).c_str());
        (*n_written)++;
    }
    log << "Faraday synthesis: " << *n_written << " of " << ch.n_records << " records of " << n_rows << " rows x " << n_chan << " channels on " << n_phi
        << " depths from " << phi0 << " in steps of " << dphi << " rad/m^2 (fwhm " << fwhm << "); left out: " << *n_left_out << " with fewer than "
        << faraday_min_baseline_rows << " baseline rows" << std::endl;
    out.keep = true;
    return BF_OK;
}

}  // namespace dsabf
