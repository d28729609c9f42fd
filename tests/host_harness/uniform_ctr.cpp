// Host build of the uniform-counter helpers of gym_art_amd/csrc/quad_core.hpp for tests/test_uniform_ctr_cpu.py: the functions gaq.hip
// advances a synchronised batch's tick / SVD word with and packs it into StepCfg::sweep with.  Test infrastructure only.
#include "../../gym_art_amd/csrc/quad_core.hpp"

extern "C" {
uint32_t uc_advance(uint32_t word, int32_t sim_steps, int32_t svd_period, int32_t ep_len, int32_t auto_reset) {
  return gaq::uniform_ctr_advance(word, sim_steps, svd_period, ep_len, auto_reset);
}
uint32_t uc_pack(uint32_t word) { return gaq::uniform_ctr_pack(word); }
uint32_t uc_unpack(uint32_t sweep) { return gaq::uniform_ctr_unpack(sweep); }
uint32_t uc_valid_bit(void) { return gaq::kUniCtrValid; }
uint32_t uc_svd_max(void) { return gaq::kUniCtrSvdMax; }
}
