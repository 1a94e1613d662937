// instantiation unit: every kernel of the N = 1 modes, P = 3 (tensor order 2) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<1, 3>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
