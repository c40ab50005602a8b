// ato_replay.hip -- the replay kernel (ato_replay.hpp), one instantiation per model variant.
#include <hip/hip_runtime.h>
#define ATO_DEFINE_REPLAY_LAUNCHER
#include "ato_replay.hpp"

namespace ato {
#define ATO_REPLAY_INST(...)                                                                                    \
    template hipError_t launch_replay<__VA_ARGS__>(const ProbD&, const ReplayD&, int, int, const double*, double*, \
                                             double*, double*, hipStream_t);
ATO_REPLAY_INST(DroneModel<ESP, GLOBAL>)
ATO_REPLAY_INST(DroneModel<ESP, PARAM_GR>)
ATO_REPLAY_INST(DroneModel<ESP, PARAM_REL>)
ATO_REPLAY_INST(DroneModel<YPR, GLOBAL>)
ATO_REPLAY_INST(DroneModel<YPR, PARAM_GR>)
ATO_REPLAY_INST(DroneModel<YPR, PARAM_REL>)
ATO_REPLAY_INST(DroneModel<DCM, GLOBAL>)
ATO_REPLAY_INST(DroneModel<DCM, PARAM_GR>)
ATO_REPLAY_INST(DroneModel<DCM, PARAM_REL>)
ATO_REPLAY_INST(PointModel<GLOBAL>)
ATO_REPLAY_INST(PointModel<PARAM_GR>)
ATO_REPLAY_INST(PointModel<PARAM_REL>)
#undef ATO_REPLAY_INST
}  // namespace ato
