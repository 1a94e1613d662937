// instantiation unit: every kernel of the N = 4 modes, P = 1 (tensor order 0) family
#include "launch_impl.hpp"
namespace cloudy {
template hipError_t launch_np<4, 1>(const HostPlan &h, const LaunchReq &r);
}  // namespace cloudy
