// The byte grammar of the text tokeniser (csrc/text_tokens.hip, K17): byte classes, the five rules that decide
// whether a token starts at a byte, the case rule and a token's length.  Host and device compile the same inline functions:
// tools/text_grammar_check.cpp runs them on the CPU, where tests/test_text_tokens_cpu.py compares them with the tests' restatement
// of the grammar.  Every function reads only bytes [t0, t1) of its text.
#pragma once
#include <stdint.h>
#include "../../include/nnl.h"

#if defined(__HIPCC__)
#define TGR_HD __host__ __device__ inline
#else
#define TGR_HD inline
#endif

namespace nnl_text_grammar {

TGR_HD bool is_space(int c) { return (c >= 9 && c <= 13) || c == 32; }
TGR_HD bool is_digit(int c) { return c >= '0' && c <= '9'; }
TGR_HD bool is_upper(int c) { return c >= 'A' && c <= 'Z'; }
TGR_HD bool is_lower(int c) { return c >= 'a' && c <= 'z'; }
// W without the digit rule: 0-9 A-Z a-z _ and every byte of a UTF-8 multibyte character
TGR_HD bool is_raw_w(int c) { return is_digit(c) || is_upper(c) || is_lower(c) || c == '_' || c >= 0x80; }
TGR_HD int to_lower(int c) { return is_upper(c) ? c + 32 : c; }

// one text [t0, t1) of the buffer; a byte outside it reads as a space, so no rule sees across a text boundary
struct TextView {
  const uint8_t* b;
  int64_t t0, t1;
  TGR_HD int at(int64_t i) const { return (i >= t0 && i < t1) ? (int)b[i] : 32; }
  TGR_HD bool special_at(int64_t i) const {      // <eos>, <bos>, <unk> begin at i
    if (i < t0 || i + 5 > t1 || b[i] != '<' || b[i + 4] != '>') return false;
    const int x = b[i + 1], y = b[i + 2], z = b[i + 3];
    return (x == 'e' && y == 'o' && z == 's') || (x == 'b' && y == 'o' && z == 's') || (x == 'u' && y == 'n' && z == 'k');
  }
  TGR_HD bool inside_special(int64_t i) const {  // one of them began 1 .. 4 bytes earlier
    return special_at(i - 1) || special_at(i - 2) || special_at(i - 3) || special_at(i - 4);
  }
  TGR_HD bool eff_w(int64_t i) const {            // W with the digit rule: 3.5 and 1,000 stay whole
    const int c = at(i);
    return is_raw_w(c) || ((c == '.' || c == ',') && is_digit(at(i - 1)) && is_digit(at(i + 1)));
  }
  TGR_HD bool apos(int64_t i) const { return at(i) == '\'' && is_raw_w(at(i - 1)) && is_raw_w(at(i + 1)); }
  TGR_HD bool nt(int64_t i) const {               // n't begins at i: n ' t and then no word byte
    const int c = at(i), t = at(i + 2);
    return (c == 'n' || c == 'N') && at(i + 1) == '\'' && (t == 't' || t == 'T') && !is_raw_w(at(i + 3));
  }
};

// tokens that start at byte i of its text: 0, 1, or 2 = the pseudo-token t_up and the token
TGR_HD int starts_at(const TextView& v, int64_t i, int mode) {
  const int c = v.at(i);
  if (is_space(c)) return 0;
  if (mode == NNL_TEXT_MODE_SPLIT) return is_space(v.at(i - 1)) ? 1 : 0;
  if (v.inside_special(i)) return 0;
  if (v.special_at(i)) return 1;
  bool start, word = false;
  if (v.nt(i)) {
    start = word = true;                                   // the word before ends one byte earlier
  } else if (c == '\'' && v.apos(i)) {
    start = !v.nt(i - 1);                                  // 's 're 'll; the apostrophe of n't belongs to n't
  } else if (v.eff_w(i)) {
    start = !(v.eff_w(i - 1) || v.apos(i - 1));
    word = is_raw_w(c);
  } else {                                                 // a run of one repeated P byte; the > that closes a special is not part of it
    start = !(v.at(i - 1) == c && !v.inside_special(i - 1));
  }
  if (!start) return 0;
  if (word && !is_raw_w(v.at(i - 1))) {                    // a run of raw W bytes begins with this token: the case rule
    bool up = false, low = false;
    int64_t j = i;
    for (; j < v.t1 && !low; ++j) {
      const int d = v.b[j];
      if (!is_raw_w(d)) break;
      up = up || is_upper(d);
      low = is_lower(d);
    }
    if (up && !low && j - i > 2) return 2;
  }
  return 1;
}

// the token that starts at i ends before the next start, whitespace or the end of the text
TGR_HD int token_length(const TextView& v, int64_t i, int mode) {
  int64_t j = i + 1;
  while (j < v.t1 && !is_space(v.b[j]) && starts_at(v, j, mode) == 0) ++j;
  return (int)(j - i);
}

}  // namespace nnl_text_grammar
