// bf_fused16_k1p16_fold_stream.hip -- the antenna-fold kernels for gemm-units of whole chunk spans (fused16_fold_stream_kernel,
// bf_fused16.hpp): n_ipo 16 / 32 / 64 x canonical, contracted and fast detect; a translation unit of their own, so that the kernel set
// and the code of bf_fused16_k1p16_fold.hip stay what they were.
#include "bf_fused16.hpp"

namespace dsabf {
namespace {
template <int NIPO>
FusedVariant fold_stream_nipo(int mode)
{
    if (mode == kDetFast) return make_fold_stream_variant<NIPO, kDetFast>();
    if (mode == kDetContracted) return make_fold_stream_variant<NIPO, kDetContracted>();
    return make_fold_stream_variant<NIPO, kDetCanonical>();
}
}  // namespace

FusedVariant fused16_variant_k1p16_fold_stream(int n_ipo, int mode)
{
    switch (n_ipo) {
        case 16: return fold_stream_nipo<16>(mode);
        case 32: return fold_stream_nipo<32>(mode);
        case 64: return fold_stream_nipo<64>(mode);
        default: return FusedVariant{};
    }
}
}  // namespace dsabf
