// like_selftest.cpp — stand-alone check of serenedb_amd/csrc/sdb_like.h, the
// matcher shared by libsdb_host.so and the HIP string kernels. Host code
// only; meant to be built with sanitizers:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined
//       -fno-sanitize-recover=all tools/like_selftest.cpp -o like_selftest
//   ./like_selftest
//
// It compiles every pattern form and every rejection, matches a handful of
// rows against each (expected verdicts written out by hand), and compares the
// matcher with a plain recursive LIKE on a small exhaustive set. Exit 0 and
// "like_selftest: ok" on success.

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../serenedb_amd/csrc/sdb_like.h"

static int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static const uint8_t* u8(const std::string& s) {
  return reinterpret_cast<const uint8_t*>(s.data());
}

// 1 / 0 = verdict, -1 = the pattern is rejected
static int like(const std::string& pat, int escape, const std::string& row) {
  SdbLikeProg* p = new SdbLikeProg;  // heap: the sanitizer sees its bounds
  int r = -1;
  if (sdb_like_compile(u8(pat), (uint32_t)pat.size(), escape, p) == 0)
    r = sdb_like_match(*p, u8(row), row.size()) ? 1 : 0;
  delete p;
  return r;
}

static int literal(const std::string& lit, bool as, bool ae,
                   const std::string& row) {
  SdbLikeProg* p = new SdbLikeProg;
  int r = -1;
  if (sdb_like_literal(u8(lit), (uint32_t)lit.size(), as, ae, p) == 0)
    r = sdb_like_match(*p, u8(row), row.size()) ? 1 : 0;
  delete p;
  return r;
}

// the textbook recursive matcher over an already well-formed pattern
static bool slow(const std::string& p, size_t i, int esc,
                 const std::string& s, size_t j) {
  if (i == p.size()) return j == s.size();
  if (esc >= 0 && (uint8_t)p[i] == esc)
    return j < s.size() && s[j] == p[i + 1] && slow(p, i + 2, esc, s, j + 1);
  if (p[i] == '%') {
    for (size_t k = j; k <= s.size(); ++k)
      if (slow(p, i + 1, esc, s, k)) return true;
    return false;
  }
  return j < s.size() && s[j] == p[i] && slow(p, i + 1, esc, s, j + 1);
}

static bool well_formed(const std::string& p, int esc) {
  for (size_t i = 0; i < p.size(); ++i) {
    if (esc >= 0 && (uint8_t)p[i] == esc) {
      if (++i >= p.size()) return false;
    } else if (p[i] == '_') {
      return false;
    }
  }
  return true;
}

int main() {
  const std::string x63(63, 'x'), x64(64, 'x');
  // forms
  CHECK(like("", -1, "") == 1 && like("", -1, "a") == 0);
  CHECK(like("%", -1, "") == 1 && like("%%%", -1, "abc") == 1);
  CHECK(like("%a%", -1, "bab") == 1 && like("%a%", -1, "bbb") == 0);
  CHECK(like("%ab", -1, "abab") == 1 && like("%ab", -1, "aba") == 0);
  CHECK(like("a%", -1, "a") == 1 && like("a%", -1, "ba") == 0);
  CHECK(like("abab", -1, "abab") == 1 && like("abab", -1, "ababa") == 0);
  CHECK(like("abab", -1, "aba") == 0);
  CHECK(like("a%a", -1, "a") == 0 && like("a%a", -1, "aa") == 1);
  CHECK(like("%ab%ab", -1, "abab") == 1 && like("%ab%ab", -1, "aba") == 0);
  CHECK(like("aba%ba", -1, "ababa") == 1 && like("aba%ba", -1, "abab") == 0);
  CHECK(like("%aab%", -1, "aaab") == 1);
  CHECK(like("%abcabd%", -1, "abcabcabd") == 1);
  CHECK(like("%a%b%c%a%b%d%", -1, "abcabd") == 1);
  CHECK(like("%" + x63 + "%", -1, "y" + x63) == 1);
  CHECK(like("%" + x63 + "%", -1, std::string(62, 'x') + "y") == 0);
  CHECK(like("%" + x63, -1, x64) == 1 && like(x63, -1, x64) == 0);
  CHECK(like(std::string("%\0%", 3), -1, std::string("a\0b", 3)) == 1);
  CHECK(like("%\xff", -1, "a\xff") == 1 && like("%\xff", -1, "\xff""a") == 0);
  // escapes
  CHECK(like("%!%%", '!', "a%b") == 1 && like("%!%%", '!', "ab") == 0);
  CHECK(like("a!_b", '!', "a_b") == 1 && like("a!_b", '!', "axb") == 0);
  CHECK(like("%!!%", '!', "a!b") == 1 && like("!a!b", '!', "ab") == 1);
  CHECK(like("%\\%", -1, "\\") == 1 && like("a\\\\b", '\\', "a\\b") == 1);
  CHECK(like("a__b", '_', "a_b") == 1);
  CHECK(like(std::string("a\0%b", 4), 0, "a%b") == 1);
  // rejections
  CHECK(like("ab!", '!', "") == -1 && like("%!", '!', "") == -1);
  CHECK(like("a_b", -1, "") == -1 && like("%_%", '!', "") == -1);
  CHECK(like(x64, -1, "") == -1);
  CHECK(like(std::string(32, 'x') + "%" + std::string(32, 'y'), -1, "") == -1);
  CHECK(like(std::string(256, '%'), -1, "") == -1);
  CHECK(like("abc", '%', "") == -1 && like("abc", 256, "") == -1);
  CHECK(like("abc", -2, "") == -1);
  {
    SdbLikeProg* p = new SdbLikeProg;  // untouched on a rejection
    std::memset(p, 0xa5, sizeof(*p));
    CHECK(sdb_like_compile(u8("a_"), 2, -1, p) == -1);
    const uint8_t* b = reinterpret_cast<const uint8_t*>(p);
    bool same = true;
    for (size_t i = 0; i < sizeof(*p); ++i) same = same && b[i] == 0xa5;
    CHECK(same);
    delete p;
  }
  // limits: 63 one-byte segments, 255 pattern bytes
  {
    std::string p, row, gaps;
    for (int i = 0; i < 63; ++i) {
      if (i) p += '%';
      p += char('a' + i % 26);
      row += char('a' + i % 26);
      gaps += char('a' + i % 26);
      gaps += "--";
    }
    CHECK(p.size() == 125);
    CHECK(like(p, -1, row) == 1 && like(p, -1, gaps) == 0);
    CHECK(like(p, -1, gaps.substr(0, gaps.size() - 2)) == 1);
    CHECK(like(p, -1, row.substr(0, 62)) == 0);
    const std::string wide = std::string(96, '%') + x63 + std::string(96, '%');
    CHECK(wide.size() == 255 && like(wide, -1, "y" + x63) == 1);
  }
  // the literal forms: EQ, PREFIX, SUFFIX, CONTAINS, and their empty cases
  CHECK(literal("ab", true, true, "ab") == 1 && literal("ab", true, true, "abc") == 0);
  CHECK(literal("ab", true, false, "abc") == 1 && literal("ab", true, false, "cab") == 0);
  CHECK(literal("ab", false, true, "cab") == 1 && literal("ab", false, true, "abc") == 0);
  CHECK(literal("ab", false, false, "cabc") == 1 && literal("ab", false, false, "acb") == 0);
  CHECK(literal("", true, true, "") == 1 && literal("", true, true, "a") == 0);
  CHECK(literal("", true, false, "a") == 1 && literal("", false, true, "a") == 1);
  CHECK(literal("", false, false, "") == 1);
  CHECK(literal(x63, false, false, "y" + x63 + "y") == 1);
  CHECK(literal(x64, false, false, "") == -1);
  // exhaustive: patterns of 0..5 and rows of 0..6 bytes over a b % !
  {
    const char alpha[] = {'a', 'b', '%', '!'};
    std::vector<std::string> pats{""}, rows{""};
    for (size_t lo = 0, n = 0; n < 6; ++n) {
      const size_t hi = rows.size();
      for (size_t i = lo; i < hi; ++i)
        for (char c : alpha) rows.push_back(rows[i] + c);
      lo = hi;
    }
    for (size_t lo = 0, n = 0; n < 5; ++n) {
      const size_t hi = pats.size();
      for (size_t i = lo; i < hi; ++i)
        for (char c : alpha) pats.push_back(pats[i] + c);
      lo = hi;
    }
    size_t pairs = 0;
    for (const std::string& p : pats) {
      SdbLikeProg prog;
      const int rc = sdb_like_compile(u8(p), (uint32_t)p.size(), '!', &prog);
      CHECK((rc == 0) == well_formed(p, '!'));
      if (rc) continue;
      for (const std::string& r : rows) {
        const bool got = sdb_like_match(prog, u8(r), r.size());
        if (got != slow(p, 0, '!', r, 0)) {
          std::fprintf(stderr, "mismatch: pattern '%s' row '%s'\n", p.c_str(),
                       r.c_str());
          ++failures;
        }
        ++pairs;
      }
    }
    std::printf("like_selftest: %zu patterns, %zu pairs\n", pats.size(), pairs);
  }
  if (failures) {
    std::fprintf(stderr, "like_selftest: %d failures\n", failures);
    return 1;
  }
  std::printf("like_selftest: ok\n");
  return 0;
}
