#include "hgp_sep_dispatch.hpp"
namespace hgp {
template int sep_pairs<float>(int);
template hipError_t launch_sep<float>(int, const SepDesc&, hipStream_t);
}
