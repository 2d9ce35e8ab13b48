// K11's per-member decoder (annotatedvdb_amd/csrc/avdb_inflate.hpp) under the host
// sanitizers: a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/bgzf_sanitize.hip -o bgzf_sanitize
//   ./bgzf_sanitize corpus.bgzf [mutations]
//
// The corpus is a chain of BGZF members (tests/test_bgzf_host.py writes the fixture
// chain and the corrupt members).  Every member is decoded from a heap copy of exactly
// its own bytes into a heap buffer of exactly its ISIZE, so a read or a write one byte
// outside either is reported; a member that decodes must agree with its own CRC (the
// decoder checks it).  Then, from a fixed seed: single-byte flips of a member (header,
// stream or trailer) and truncations of it, each decoded the same way — any status is
// fine, any sanitizer report is not.  Exit status 0 and a last line "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_inflate.hpp"

#include "sanitize_common.hpp"

#include <string.h>

using namespace avdb;

static const uint8_t kSentinel = 0xA5;

// decode `bytes` of a member (a heap copy of exactly that size) that states `isize`;
// the status, or -1 if a byte outside an OK member's output changed
static int decode(inflate::State& S, inflate::Window& W, const uint8_t* member, size_t bytes, uint32_t isize, bool* ok) {
  auto in = exact<uint8_t>(bytes);
  memcpy(in.get(), member, bytes);
  auto out = exact<uint8_t>(isize);
  memset(out.get(), kSentinel, isize ? isize : 1);
  const uint32_t st = inflate::inflate_member(inflate::Lanes{0, 1}, S, W.b, in.get(), bytes, 0, 0, isize, out.get(), isize);
  *ok = st == AVDB_BGZF_OK;
  if (st != AVDB_BGZF_OK)
    for (uint32_t i = 0; i < isize; ++i)
      if (out[i] != kSentinel) return -1;
  return int(st);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s corpus.bgzf [mutations]\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> data = read_file(argv[1]);
  const long mutations = argc > 2 ? atol(argv[2]) : 2000;

  struct Span {
    size_t at;
    inflate::Member m;
  };
  std::vector<Span> members;
  for (size_t at = 0; at < data.size();) {
    inflate::Member m;
    if (inflate::parse_member(data.data() + at, data.size() - at, &m) != inflate::kMemberOk) {
      fprintf(stderr, "no BGZF member at offset %zu of the corpus\n", at);
      return 2;
    }
    members.push_back(Span{at, m});
    at += m.total_bytes;
  }
  std::unique_ptr<inflate::State> S(new inflate::State());
  std::unique_ptr<inflate::Window> W(new inflate::Window());
  size_t n_ok = 0;
  unsigned long by_status[16] = {};
  for (const Span& s : members) {
    bool ok;
    const int st = decode(*S, *W, data.data() + s.at, s.m.total_bytes, s.m.isize, &ok);
    if (st < 0) {
      fprintf(stderr, "member at %zu failed but wrote output\n", s.at);
      return 1;
    }
    n_ok += ok;
  }
  printf("%zu of %zu members OK\n", n_ok, members.size());

  std::vector<uint8_t> work;
  for (long it = 0; it < mutations; ++it) {
    // every other time the member that holds a random byte of the corpus (the long streams), else any member
    size_t pick = rnd() % members.size();
    if (it & 1) {
      const size_t byte = rnd() % data.size();
      for (pick = 0; pick + 1 < members.size() && members[pick + 1].at <= byte;) ++pick;
    }
    const Span& s = members[pick];
    work.assign(data.begin() + s.at, data.begin() + s.at + s.m.total_bytes);
    size_t bytes = work.size();
    const uint64_t kind = rnd() % 8;
    if (kind == 0) {
      bytes = rnd() % (work.size() + 1);  // truncated: the caller's buffer ends inside the member
    } else if (kind == 1 && s.m.total_bytes > s.m.hdr_bytes + 9) {
      // a shorter stream with BSIZE and the trailer moved to match (the first subfield is BC in the corpus' members
      // but one; there the flip below is what happens)
      const size_t cut = 1 + rnd() % (s.m.total_bytes - s.m.hdr_bytes - 9);
      if (work[12] == 'B' && work[13] == 'C') {
        memmove(work.data() + work.size() - 8 - cut, work.data() + work.size() - 8, 8);
        bytes = work.size() - cut;
        work[16] = uint8_t((bytes - 1) & 0xFF);
        work[17] = uint8_t((bytes - 1) >> 8);
      }
    } else {
      const int flips = kind == 2 ? 3 : 1;
      for (int f = 0; f < flips; ++f) work[rnd() % work.size()] ^= uint8_t(1u << (rnd() % 8));
    }
    bool ok;
    const int st = decode(*S, *W, work.data(), bytes, s.m.isize, &ok);
    if (st < 0) {
      fprintf(stderr, "mutation %ld of the member at %zu failed but wrote output\n", it, s.at);
      return 1;
    }
    ++by_status[st & 15];
  }
  printf("%ld mutations, by status:", mutations);
  for (int k = 0; k < 11; ++k) printf(" %d:%lu", k, by_status[k]);
  printf("\nclean\n");
  return 0;
}
