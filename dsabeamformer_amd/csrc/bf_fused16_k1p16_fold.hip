// bf_fused16_k1p16_fold.hip -- the antenna-fold kernels (fused16_fold_kernel, bf_fused16.hpp): 64 mirror-symmetric antennas,
// n_ipo 16 / 32 / 64 x canonical, contracted and fast detect; a translation unit of their own so that they compile beside the classes.
#include "bf_fused16.hpp"

namespace dsabf {
namespace {
template <int NIPO>
FusedVariant fold_nipo(int mode)
{
    if (mode == kDetFast) return make_fold_variant<NIPO, kDetFast>();
    if (mode == kDetContracted) return make_fold_variant<NIPO, kDetContracted>();
    return make_fold_variant<NIPO, kDetCanonical>();
}
}  // namespace

FusedVariant fused16_variant_k1p16_fold(int n_ipo, int mode)
{
    switch (n_ipo) {
        case 16: return fold_nipo<16>(mode);
        case 32: return fold_nipo<32>(mode);
        case 64: return fold_nipo<64>(mode);
        default: return FusedVariant{};
    }
}
}  // namespace dsabf
