// instantiation unit: every kernel of the N = 4 modes, P = 4 (tensor order 3) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<4, 4>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
