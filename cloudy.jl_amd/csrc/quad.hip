// instantiation unit: the NumericalCoalStyle (fixed Gauss rule, converged mode) kernels of one N mode family.  The
// Makefile compiles it once per N, quad_n<N>.o, with -DCLOUDY_INST_N=<N>; host_plan.hpp declares launch_quad_n<N>.
#if !defined(CLOUDY_INST_N)
#error "compile through the Makefile: it passes -DCLOUDY_INST_N=<N> for each family"
#endif
#include "launch_quad_impl.hpp"
// launch_quad_n<N>: two macro levels, because an argument next to ## is pasted before it is expanded
#define CLOUDY_QUAD_ENTRY_(n) launch_quad_n##n
#define CLOUDY_QUAD_ENTRY(n) CLOUDY_QUAD_ENTRY_(n)
namespace cloudy {
hipError_t CLOUDY_QUAD_ENTRY(CLOUDY_INST_N)(const HostPlan &h, const LaunchReq &r) {
    return launch_quad<CLOUDY_INST_N>(h, r);
}
}  // namespace cloudy
#undef CLOUDY_QUAD_ENTRY
#undef CLOUDY_QUAD_ENTRY_
