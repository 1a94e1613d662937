// instantiation unit: every kernel of the N = 2 modes, P = 5 (tensor order 4) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<2, 5>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
