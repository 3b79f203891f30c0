// Sanitizer run of trgt_amd/csrc/inflate_fast.hpp on the hand-made streams of tests/deflate_builder.py (the paths zlib's compressor never
// emits), against zlib's inflate, in exact-size heap buffers.  Build and run (from tests/tools):
//   python ../deflate_builder.py --dump /tmp/inflate_vectors.bin
//   g++ -O1 -g -fsanitize=address,undefined -std=c++17 inflate_vectors_asan.cpp -lz -o /tmp/inflate_vectors_asan && ASAN_OPTIONS=detect_leaks=0 /tmp/inflate_vectors_asan /tmp/inflate_vectors.bin
// A record of the dump: u32 n_in, u32 n_out, u8 accept (1: a valid stream the decoder must take; 0: malformed, wrongly announced, or of a
// class it leaves to zlib), the stream.  wrong: accepted bytes that are not zlib's, or a verdict other than the record's.
// Last run: 357 cases, 265 accepted, 92 declined (90 malformed or wrongly announced, 2 of the classes left to zlib), 0 wrong, no sanitizer report.
#include "../../trgt_amd/csrc/inflate_fast.hpp"
#include <zlib.h>
#include <vector>
#include <cstdio>
#include <cstdlib>
using namespace trgt::inflate_fast;
static bool zinflate(const uint8_t* in, size_t n, std::vector<uint8_t>& out, size_t want) {
  z_stream zs; memset(&zs, 0, sizeof zs); inflateInit2(&zs, -15);
  out.assign(want + 1, 0);
  zs.next_in = (Bytef*)in; zs.avail_in = n; zs.next_out = out.data(); zs.avail_out = want + 1;
  int rc = inflate(&zs, Z_FINISH); size_t got = zs.total_out; inflateEnd(&zs);
  out.resize(got); return rc == Z_STREAM_END && got == want;
}
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s DUMP\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  Tables* T = new Tables();
  long ok = 0, declined = 0, bad = 0, cases = 0;
  for (;;) {
    uint32_t hdr[2]; uint8_t accept;
    if (fread(hdr, 4, 2, f) != 2 || fread(&accept, 1, 1, f) != 1) break;
    const size_t n_in = hdr[0], want = hdr[1];
    // exact-size heap copies so that ASan sees any access beyond either buffer
    uint8_t* in = (uint8_t*)malloc(n_in ? n_in : 1);
    if (fread(in, 1, n_in, f) != n_in) { fprintf(stderr, "short record %ld\n", cases); return 2; }
    uint8_t* out = (uint8_t*)malloc(want ? want : 1);
    const bool r = inflate_block(in, n_in, out, want, *T);
    std::vector<uint8_t> ref;
    const bool zr = zinflate(in, n_in, ref, want);
    if (r) {
      if (!zr || memcmp(ref.data(), out, want) != 0) { ++bad; fprintf(stderr, "MISMATCH case %ld n_in=%zu n_out=%zu zr=%d\n", cases, n_in, want, (int)zr); }
      else if (!accept) { ++bad; fprintf(stderr, "ACCEPTED case %ld that must be declined\n", cases); }
      else ++ok;
    } else {
      ++declined;
      if (accept) { ++bad; fprintf(stderr, "DECLINED case %ld n_in=%zu n_out=%zu zr=%d\n", cases, n_in, want, (int)zr); }
    }
    ++cases;
    free(in); free(out);
  }
  fclose(f);
  printf("cases %ld accepted %ld declined %ld wrong %ld\n", cases, ok, declined, bad);
  return bad != 0;
}
