// block_data_host.cpp -- the host baseline of scripts/block_data_bench.py: a
// BLOCK_DATA run parsed serially (parse_data_run, sf_wire_data.hpp) and every
// payload hashed with sf_sha1_host and compared with its claimed digest, on
// the calling thread.  The script builds it as a small shared object beside
// the library:
//   g++ -O2 -std=c++17 -shared -fPIC block_data_host.cpp -L../syncfast_amd/lib -lsyncfast_amd
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../include/syncfast_amd.h"
#include "../syncfast_amd/csrc/sf_wire_data.hpp"

extern "C" int block_data_host(const uint8_t* run, uint64_t n, uint64_t* n_msgs, uint64_t* n_bad) {
  const uint64_t most = n / sfwp::kMinData + 1;
  std::vector<uint8_t> digests(most * 20);
  std::vector<uint32_t> sizes(most);
  std::vector<uint64_t> offsets(most);
  uint64_t consumed = 0, need = 0;
  int stop = 0;
  bool too_large = false;
  sfwp::parse_data_run(run, n, digests.data(), sizes.data(), offsets.data(), most, n_msgs, &consumed, &stop, &need,
                       &too_large);
  *n_bad = 0;
  for (uint64_t i = 0; i < *n_msgs; i++) {
    uint8_t d[20];
    const int rc = sf_sha1_host(run + offsets[i], sizes[i], d);
    if (rc != SF_OK) return rc;
    *n_bad += memcmp(d, digests.data() + 20 * i, 20) != 0;
  }
  return stop;
}
