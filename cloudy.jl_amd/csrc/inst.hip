// instantiation unit: every kernel of one family (N modes, P = tensor order + 1).  The Makefile compiles it once per
// family, inst_n<N>_p<P>.o, with -DCLOUDY_INST_N=<N> -DCLOUDY_INST_P=<P>, so that the families compile in parallel.
#if !defined(CLOUDY_INST_N) || !defined(CLOUDY_INST_P)
#error "compile through the Makefile: it passes -DCLOUDY_INST_N=<N> -DCLOUDY_INST_P=<P> for each family"
#endif
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<CLOUDY_INST_N, CLOUDY_INST_P>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
