// Host-only walk of the tokeniser's byte grammar (neuralnetworklibrary_amd/csrc/text_grammar.h, the functions the kernels of
// csrc/text_tokens.hip compile for the device): prints the token records of a corpus, one "start len" line per token in byte order,
// the pseudo-token t_up as len -1.  tests/test_text_tokens_cpu.py builds it and compares its output with the tests' restatement of
// the grammar, so the rules are checked on a machine without a GPU.  Build and run (from the repository root):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/text_grammar_check.cpp -o text_grammar_check
//   ./text_grammar_check MODE BYTES_FILE OFFSETS_FILE      (MODE 0 = grammar, 1 = split; OFFSETS_FILE: n + 1 decimal offsets)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../neuralnetworklibrary_amd/csrc/text_grammar.h"

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s MODE BYTES_FILE OFFSETS_FILE\n", argv[0]);
    return 2;
  }
  const int mode = std::atoi(argv[1]);
  std::vector<uint8_t> bytes;
  if (FILE* f = std::fopen(argv[2], "rb")) {
    int c;
    while ((c = std::fgetc(f)) != EOF) bytes.push_back((uint8_t)c);
    std::fclose(f);
  } else {
    return 2;
  }
  std::vector<long long> off;
  if (FILE* f = std::fopen(argv[3], "r")) {
    long long v;
    while (std::fscanf(f, "%lld", &v) == 1) off.push_back(v);
    std::fclose(f);
  } else {
    return 2;
  }
  if (off.size() < 2 || off.front() != 0 || off.back() != (long long)bytes.size()) return 2;
  bytes.push_back(0);      // so that data() is never null for an empty corpus; never read: every view ends before it
  for (size_t j = 0; j + 1 < off.size(); ++j) {
    if (off[j] > off[j + 1]) return 2;
    const nnl_text_grammar::TextView v{bytes.data(), off[j], off[j + 1]};
    for (int64_t i = v.t0; i < v.t1; ++i) {
      const int c = nnl_text_grammar::starts_at(v, i, mode);
      if (c == 2) std::printf("%lld %d\n", (long long)i, NNL_TEXT_TUP_LEN);
      if (c >= 1) std::printf("%lld %d\n", (long long)i, nnl_text_grammar::token_length(v, i, mode));
    }
  }
  return 0;
}
