// The launch record of the stage launchers (bf_launch_record.h) and its C entry point bf_stage_launches (include/dsabf_bench.h).
#include "bf_launch_record.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "dsabf_bench.h"

namespace dsabf {
namespace {

struct Ring {
    const char* name[kLaunchRecordSlots];
    char text[kLaunchRecordSlots][kLaunchRecordChars];
    unsigned long long count;   // names recorded since the last clear
};

thread_local Ring ring;

}  // namespace

void record_launch(const char* literal)
{
    ring.name[ring.count++ % kLaunchRecordSlots] = literal;
}

void record_launchf(const char* fmt, ...)
{
    const unsigned slot = (unsigned)(ring.count++ % kLaunchRecordSlots);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ring.text[slot], kLaunchRecordChars, fmt, ap);
    va_end(ap);
    ring.name[slot] = ring.text[slot];
}

}  // namespace dsabf

extern "C" int bf_stage_launches(char* buf, size_t buflen, int clear)
{
    using namespace dsabf;
    if (!buf || buflen == 0) return BF_ERR_INVALID;
    const unsigned long long n = ring.count < (unsigned long long)kLaunchRecordSlots ? ring.count : kLaunchRecordSlots;
    size_t need = 1;
    for (unsigned long long i = ring.count - n; i < ring.count; i++) need += strlen(ring.name[i % kLaunchRecordSlots]) + 1;
    if (need > buflen) return BF_ERR_INVALID;
    char* p = buf;
    for (unsigned long long i = ring.count - n; i < ring.count; i++) {
        const char* s = ring.name[i % kLaunchRecordSlots];
        const size_t len = strlen(s);
        memcpy(p, s, len);
        p += len;
        *p++ = '\n';
    }
    *p = 0;
    if (clear) ring.count = 0;
    return BF_OK;
}
