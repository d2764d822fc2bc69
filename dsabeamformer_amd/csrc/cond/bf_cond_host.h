// bf_cond_host.h -- what the runtime's translation units share about the conditioning stage (bf_cond.cpp, bf_dm_stream.cpp,
// bf_runtime.cpp).  Host-only and not installed; no .hip file includes it.
#pragma once
#include "../bf_runtime_internal.h"

#pragma GCC visibility push(hidden)
namespace dsabf::rt {

// bf_cond.cpp
void cond_release_handle(bf_handle* h);   // bf_destroy: the device side of every conditioner of `h` goes; the objects stay, detached from it
int cond_check_attach(const struct bf_cond* c, const bf_handle* h, int n_freq_total, int max_rows);   // bf_dm_stream_attach_conditioner's conditions
void cond_set_feeder(struct bf_cond* c, struct bf_dm_stream* dm);   // the DM stage that pushes into `c` (NULL: none): told when `c` is destroyed
// bf_dm_stream.cpp
void dm_stream_drop_conditioner(struct bf_dm_stream* s);            // the conditioner attached to `s` is going away

}  // namespace dsabf::rt
#pragma GCC visibility pop
