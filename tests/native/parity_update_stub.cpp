// For parity_test.cpp's program, which has no GPU path.
#include "hipstore/parity.h"

namespace hipstore {
int parity_update_gpu(int, const ParitySet&, const ParitySet&, uint8_t*,
                      uint8_t*, uint64_t, uint32_t, bool,
                      std::vector<uint64_t>*) {
  return kIoFailed;
}
}  // namespace hipstore
