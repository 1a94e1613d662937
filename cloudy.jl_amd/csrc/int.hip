// instantiation unit: the fused integrators of one family (N modes, P = tensor order + 1).  The Makefile compiles it
// once per family, int_n<N>_p<P>.o, with -DCLOUDY_INST_N=<N> -DCLOUDY_INST_P=<P> and machine LICM off
// (launch_int_impl.hpp says why).
#if !defined(CLOUDY_INST_N) || !defined(CLOUDY_INST_P)
#error "compile through the Makefile: it passes -DCLOUDY_INST_N=<N> -DCLOUDY_INST_P=<P> for each family"
#endif
#include "launch_int_impl.hpp"
namespace cloudy {
template hipError_t launch_int<CLOUDY_INST_N, CLOUDY_INST_P>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
