// bf_cdd_host.cpp -- host mirror of coherent dedispersion (include/dsabf_host.hpp: coherent_options, read_voltage_header,
// coherent_voltage_file; docs/COHERENT_DEDISPERSION.md section 5): `beam --coherent` -- every record of a --voltages file through
// bf_stokes_voltages_device and bf_cdd_stokes_device, into a file of coherently dedispersed Stokes parameters.
#include <hip/hip_runtime.h>

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

// device memory of one call, freed when it returns; the caller's current device is put back (as in bf_cal_host.cpp: bf_host_internal.h,
// where a shared copy would live, is one of the files build.kernel_build_id() hashes, and this change leaves that id alone)
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

struct stage_guard {
    bf_handle* h = nullptr;
    bf_stokes* s = nullptr;
    bf_cdd* c = nullptr;
    ~stage_guard()
    {
        if (c) bf_cdd_destroy(c);
        if (s) bf_stokes_destroy(s);
        if (h) bf_destroy(h);
    }
};

}  // namespace

bool read_voltage_header(const char* path, voltage_file_header* out, std::string* why)
{
    file_guard f{fopen(path, "rb")};
    char text[voltage_file_sink::kHeaderBytes + 1] = {0};
    if (!f.fp || fread(text, 1, voltage_file_sink::kHeaderBytes, f.fp) != voltage_file_sink::kHeaderBytes) {
        *why = std::string(path) + ": cannot read a " + std::to_string(voltage_file_sink::kHeaderBytes) + "-byte header";
        return false;
    }
    std::map<std::string, std::string> kv;
    std::istringstream lines(text);
    for (std::string line; std::getline(lines, line);) {
        const size_t sp = line.find(' ');
        if (sp != std::string::npos) kv[line.substr(0, sp)] = line.substr(sp + 1);
    }
    auto num = [&kv](const char* key) { return kv.count(key) ? atoi(kv[key].c_str()) : -1; };
    *out = voltage_file_header();
    out->n_ant = num("NANT"), out->n_freq = num("NFREQ"), out->n_pol = num("NPOL"), out->n_avg = num("NAVG"), out->n_out = num("NOUT");
    out->units = num("UNITS"), out->first_channel = num("FIRST_CHANNEL");
    if (kv["CONTENT"] != "voltages" || kv["DTYPE"] != "packed4+4" || num("HDR_SIZE") != (int)voltage_file_sink::kHeaderBytes ||
        num("RECORD_HEADER_BYTES") != (int)voltage_file_sink::kRecordBytes || out->n_ant < 1 || out->n_freq < 1 || out->n_pol != 2 || out->n_avg < 1 ||
        out->n_out < 1 || out->units < 1 || out->first_channel < 0) {
        *why = std::string(path) + " is not a file of two-polarisation voltage cuts (beam --voltages)";
        return false;
    }
    out->record_bytes = (size_t)out->units * out->n_freq * out->n_out * out->n_avg * out->n_pol * out->n_ant;
    fseek(f.fp, 0, SEEK_END);
    const long size = ftell(f.fp);
    out->n_records = size < 0 ? 0 : ((size_t)size - voltage_file_sink::kHeaderBytes) / (voltage_file_sink::kRecordBytes + out->record_bytes);
    return true;
}

int coherent_fft_length(int n_edge)
{
    for (int n = 256; n <= 4096; n *= 2)
        if (n_edge <= n / 4) return n;
    return 0;
}

int coherent_voltage_file(const coherent_options& o, uint64_t* n_written, uint64_t* n_refused, std::ostream& log)
{
    *n_written = *n_refused = 0;
    voltage_file_header vh;
    std::string why;
    if (!read_voltage_header(o.voltages_path, &vh, &why)) return set_error(BF_ERR_INVALID, why.c_str());
    bf_config cfg;
    bf_config_default(&cfg, /*debug=*/0);
    cfg.n_ant = vh.n_ant, cfg.n_freq = vh.n_freq, cfg.n_pol = vh.n_pol, cfg.n_avg = vh.n_avg, cfg.n_out_per_gemm = vh.n_out;
    const int S = vh.n_out * vh.n_avg, n_time = vh.units * S;
    // the ladder of the run that wrote the file: -M and -N as given to it
    std::vector<double> dms = dm_trials(0.0, o.dm_max);
    if (o.n_dm_cap > 0 && (int)dms.size() > o.n_dm_cap) {
        std::vector<double> pick;
        for (int i = 0; i < o.n_dm_cap; i++) pick.push_back(dms[(size_t)((double)i * (dms.size() - 1) / (o.n_dm_cap > 1 ? o.n_dm_cap - 1 : 1))]);
        dms.swap(pick);
    }
    std::vector<double> freq((size_t)vh.n_freq);
    for (int c = 0; c < vh.n_freq; c++) freq[(size_t)c] = (double)channel_frequency_weights(o.gpu, vh.first_channel + c);
    const double bw_mhz = (double)vh.n_avg / (1000.0 * o.tsamp_ms);   // a voltage sample is tsamp / n_avg long

    device_scratch mem;
    stage_guard g;
    hipError_t e = mem.begin(o.device);
    if (e != hipSuccess) return hip_fail("coherent_voltage_file", e);
    int rc = bf_create(&cfg, o.device, &g.h);
    if (rc != BF_OK) return rc;
    std::vector<int8_t> w((size_t)cfg.n_freq * cfg.n_ant * cfg.n_beams * 2);
    generate_fourier_coefficients(cfg.n_beams, cfg.n_ant, cfg.n_freq, vh.first_channel, o.gpu, o.pos, o.dir, w.data());
    if (o.gains && (rc = set_weights_conditioned(g.h, o.device, w.data(), o.gains, nullptr, w.data(), o.ant_flags)) != BF_OK) return rc;
    if ((rc = bf_stokes_create(g.h, 1, 1, &g.s)) != BF_OK) return rc;

    const size_t n_cells = (size_t)(n_time / (o.n_int > 0 ? o.n_int : 1)) * vh.n_freq * 4;
    uint8_t* d_packed = nullptr;
    float *d_volts = nullptr, *d_out = nullptr;
    if ((e = mem.alloc(&d_packed, vh.record_bytes)) != hipSuccess || (e = mem.alloc(&d_volts, (size_t)vh.n_freq * 2 * n_time * 2 * sizeof(float))) != hipSuccess ||
        (e = mem.alloc(&d_out, n_cells * sizeof(float))) != hipSuccess)
        return hip_fail("coherent_voltage_file", e);

    file_guard in{fopen(o.voltages_path, "rb")}, out{fopen(o.out_path, "wb")};
    if (!in.fp || !out.fp) return set_error(BF_ERR_INVALID, (std::string("cannot open ") + (in.fp ? o.out_path : o.voltages_path)).c_str());
    char header[coherent_file_header_bytes] = {0};
    snprintf(header, sizeof header,
             "HDR_SIZE %zu\nCONTENT coherent_stokes\nDTYPE float32\nNFREQ %d\nFIRST_CHANNEL %d\nNFFT %d\nNINT %d\nSIDEBAND %d\nNTIME %d\nNANT %d\nNAVG %d\n"
             "NOUT %d\nUNITS %d\nLAYOUT time,freq,iquv\nRECORD_HEADER_BYTES %zu\n",
             coherent_file_header_bytes, vh.n_freq, vh.first_channel, o.n_fft, o.n_int, o.sideband, n_time, vh.n_ant, vh.n_avg, vh.n_out, vh.units,
             coherent_record_header_bytes);
    if (fwrite(header, 1, sizeof header, out.fp) != sizeof header) return set_error(BF_ERR_INVALID, (std::string("cannot write ") + o.out_path).c_str());
    fseek(in.fp, (long)voltage_file_sink::kHeaderBytes, SEEK_SET);

    std::vector<uint8_t> packed(vh.record_bytes);
    std::vector<float> cells(n_cells), table;
    int have_fft = 0, have_edge = -1;
    uint64_t no_length = 0, too_short = 0, bad_trial = 0, bad_window = 0;
    for (size_t r = 0; r < vh.n_records; r++) {
        uint64_t t0;
        int32_t ints[3];
        double snr;
        if (fread(&t0, 8, 1, in.fp) != 1 || fread(ints, 4, 3, in.fp) != 3 || fread(&snr, 8, 1, in.fp) != 1 ||
            fread(packed.data(), 1, packed.size(), in.fp) != packed.size())
            return set_error(BF_ERR_INVALID, (std::string(o.voltages_path) + ": short record").c_str());
        const int trial = ints[0], beam = ints[1];
        if (trial < 0 || trial >= (int)dms.size() || beam < 0 || beam >= cfg.n_beams) {
            bad_trial++;
            continue;
        }
        const double dm = dms[(size_t)trial];
        const int n_edge = bf_cdd_edge(dm, freq.data(), vh.n_freq, bw_mhz);
        const int n_fft = o.n_fft ? o.n_fft : coherent_fft_length(n_edge);
        if (n_edge < 0 || !n_fft || n_edge > n_fft / 4) {
            no_length++;
            continue;
        }
        const int V = n_fft - 2 * n_edge;
        if (n_time < V) {
            too_short++;
            continue;
        }
        if (V % o.n_int || n_time % o.n_int) {
            bad_window++;
            continue;
        }
        table.resize((size_t)vh.n_freq * n_fft * 2);
        if ((rc = bf_cdd_chirp(dm, freq.data(), vh.n_freq, bw_mhz, o.sideband, n_fft, table.data())) != BF_OK) return rc;
        if (g.c && (n_fft != have_fft || n_edge != have_edge)) {
            bf_cdd_destroy(g.c);
            g.c = nullptr;
        }
        if (!g.c) {
            if ((rc = bf_cdd_create(g.h, vh.n_freq, n_fft, n_edge, table.data(), &g.c)) != BF_OK) return rc;
            have_fft = n_fft, have_edge = n_edge;
        } else if ((rc = bf_cdd_set_chirp(g.c, table.data())) != BF_OK) {
            return rc;
        }
        if ((rc = bf_stokes_set_weights(g.s, w.data(), &beam, 1)) != BF_OK) return rc;
        if ((e = hipMemcpy(d_packed, packed.data(), packed.size(), hipMemcpyHostToDevice)) != hipSuccess) return hip_fail("coherent_voltage_file", e);
        if ((rc = bf_stokes_voltages_device(g.s, d_packed, vh.units, d_volts, nullptr)) != BF_OK) return rc;
        if ((rc = bf_cdd_stokes_device(g.c, d_volts, 1, n_time, o.n_int, d_out, nullptr)) != BF_OK) return rc;
        if ((e = hipMemcpy(cells.data(), d_out, n_cells * sizeof(float), hipMemcpyDeviceToHost)) != hipSuccess) return hip_fail("coherent_voltage_file", e);
        const int32_t tail[2] = {n_edge, n_fft};
        if (fwrite(&t0, 8, 1, out.fp) != 1 || fwrite(ints, 4, 3, out.fp) != 3 || fwrite(&snr, 8, 1, out.fp) != 1 || fwrite(&dm, 8, 1, out.fp) != 1 ||
            fwrite(tail, 4, 2, out.fp) != 2 || fwrite(cells.data(), sizeof(float), n_cells, out.fp) != n_cells)
            return set_error(BF_ERR_INVALID, (std::string("cannot write ") + o.out_path).c_str());
        (*n_written)++;
    }
    *n_refused = no_length + too_short + bad_trial + bad_window;
    log << "Coherent dedispersion: " << *n_written << " of " << vh.n_records << " cuts of " << n_time << " samples x " << vh.n_freq << " channels, windows of "
        << o.n_int << " samples; refused: " << no_length << " with no FFT length <= 4096 for their edge, " << too_short << " shorter than one segment, "
        << bad_trial << " with a trial or beam outside the run's, " << bad_window << " whose segment the window does not divide" << std::endl;
    return BF_OK;
}

}  // namespace dsabf
