// Which stage kernel did a call launch?  Every launch site under csrc/<stage>/ names the kernel it is about to launch, spelled as the
// demangled `__device_stub__` symbol spells its template arguments ("cdd_kernel<9, true>", "vcut_kernel<unsigned int>", "corr_kernel"):
// the launchers pick among ~100 instantiations on antenna count, FFT length, alignment and the chip's CU count, and only the launcher
// knows which one it took.  The record is a thread-local ring of the most recent kLaunchRecordSlots names; a launch pays one pointer
// store (record_launch: a string literal) or one short snprintf into the slot's own text (record_launchf).  No allocation, no lock,
// nothing read from the environment.  Host code only; bf_stage_launches (include/dsabf_bench.h) reads it.
#pragma once

namespace dsabf {

constexpr int kLaunchRecordSlots = 32;
constexpr int kLaunchRecordChars = 64;

void record_launch(const char* literal);                                              // `literal` must outlive the ring: a string literal
void record_launchf(const char* fmt, ...) __attribute__((format(printf, 1, 2)));      // names longer than 63 characters are cut

}  // namespace dsabf
