// instantiation unit: every kernel of the N = 2 modes, P = 2 (tensor order 1) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<2, 2>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
