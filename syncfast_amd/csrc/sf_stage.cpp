// sf_stage.cpp -- the parts of sf_stage.hpp that need the HIP runtime or the
// knobs.  HIP runtime API only: built with the host compiler.
#include "sf_stage.hpp"

#include "sf_internal.hpp"

namespace sfi {

unsigned pool_threads(uint64_t items) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  return (unsigned)std::min<uint64_t>(std::min(io_threads(), hw), std::max<uint64_t>(1, items));
}

int stage_bufs(HostLease& res, int b, uint64_t data_bytes, uint64_t blocks, uint64_t aux_bytes, StageBufs* s) {
  int rc = SF_OK;
  if (data_bytes != kNoBuf && (rc = res.dev(kSlotData + b, data_bytes, &s->ddata)) == SF_OK)
    rc = res.pin(kSlotData + b, data_bytes, &s->pin);
  if (rc == SF_OK && blocks != kNoBuf && (rc = res.dev(kSlotDigests + b, blocks * 20, &s->ddig)) == SF_OK)
    rc = res.pin(kSlotDigests + b, blocks * 20, &s->pdig);
  if (rc == SF_OK && aux_bytes != kNoBuf && (rc = res.dev(kSlotAux + b, aux_bytes, &s->daux)) == SF_OK)
    rc = res.pin(kSlotAux + b, aux_bytes, &s->paux);
  return rc;
}

}  // namespace sfi
