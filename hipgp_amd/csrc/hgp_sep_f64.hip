#include "hgp_sep_dispatch.hpp"
namespace hgp {
template int sep_pairs<double>(int);
template hipError_t launch_sep<double>(int, const SepDesc&, hipStream_t);
}
