// instantiation unit: every kernel of the N = 2 modes, P = 3 (tensor order 2) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<2, 3>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
