// trgt_amd/csrc/bgzf_block.hpp -- what the writer (writers.hip) and the record engine (bam_records_dev.hip) must agree on about a BGZF
// block whose payload the device deflated.  Host code only, no HIP.
#pragma once
#include <cstdint>

namespace trgt {

// "the device took this block": it left a payload, and header (18) + payload + CRC-32 and size (8) fit the 64 KiB of a BGZF block.
// Any other block of the flush was declined and goes to zlib.
constexpr bool bgzf_payload_fits(uint32_t len) { return len > 0 && len + 26u <= 0x10000u; }

}  // namespace trgt
