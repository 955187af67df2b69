// The module-facing surface of a NeusTestbed. An operator module (operators.cpp) owns a private testbed as its core: the
// grids' tables, the parameter layout, the progressive-level settings, the scatter workspace and, for the NerfNetwork
// module, the NeuS network kernels. The modules see the type only as declared here; testbed.cpp, which defines it,
// forwards each function to the member of the same name.
#pragma once
#include "kernels.h"
#include "../../include/neus2_hip.h"

#include <vector>

struct NeusTestbed;

namespace neus {

struct Layout {
	uint32_t din, W, L;
	uint32_t off_d0, off_d1, off_r0, off_r1, off_r2, n_density, n_rgb, n_matrix, grid_off, n_grid, var_off, P;
};

// The members of a core the modules use, bound once by core_create. What a module may write is not const: the stream
// (StreamSwap, for the duration of a call) and the training buffers' indeed_batch / dpos around net_backward.
struct Core {
	NeusTestbed& tb;
	const int& device;
	hipStream_t& stream;
	const NeusNetworkConfig& cfg;
	const Layout& lay;
	const GridLevels& gl;
	const ScatterWork& swork;
	uint8_t* const& scan_tmp;  // scan_tmp.p, scan_tmp_bytes of it for the scatter
	const size_t& scan_tmp_bytes;
	half_t* const& params_h;   // params_h.p: fp16 [lay.P]
	TrainBufs& tbuf;
};
Core* core_create(int device);  // a full NeusTestbed on the device, with its own streams
void core_destroy(Core* c);

void setup_network(NeusTestbed& tb, const NeusNetworkConfig& c, const float* geo, bool with_mlp = true);
// a general grid sets up no network: only cfg, and lay.L, for valid_level_at and the hyper-parameters
void core_set_levels(NeusTestbed& tb, const NeusNetworkConfig& c);
void prepare_weights(NeusTestbed& tb);
std::vector<float> initial_params_rng(const NeusTestbed& tb, pcg32 rnd, const float* geo);
uint32_t valid_level_at(const NeusTestbed& tb, int step);
void net_forward(NeusTestbed& tb, const uint32_t* n_ptr, uint32_t n_fixed, uint32_t n_cap, const float* c, uint32_t valid, half_t* out, hipStream_t s);
// forward recompute + backward into g (fp32 [P], zeroed by the caller)
void net_backward(NeusTestbed& tb, const uint32_t* n_valid_ptr, const uint32_t* n_train_ptr, uint32_t n, const float* c, uint32_t valid,
                  const half_t* dlo, float* g, hipStream_t s);

} // namespace neus
