// Stand-alone host program over the P-384 headers (minbft_amd/csrc/p384_fe.h,
// p384_ecc.h) and the class's launch plan (verify_plan.h), driven by
// tests/test_p384_host.py: reads the vector file named on the command line
// (standard input without one), one command a line with its operands as hex
// integers, and prints one result line per command.  The same command set runs
// on the device through tests/csrc/p384_check.hip, which includes
// p384_check_ops.inc as well.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../minbft_amd/csrc/p384_ecc.h"
#include "../../minbft_amd/csrc/verify_plan.h"
#include "p384_check_ops.inc"

using namespace mbft;

// a hex integer below 2^448 -> 14 little-endian words
static bool parse_hex(const char* s, uint32_t w[P384_OP_WORDS]) {
  memset(w, 0, 4 * P384_OP_WORDS);
  const size_t n = strlen(s);
  if (n == 0 || n > 8 * P384_OP_WORDS) return false;
  for (size_t i = 0; i < n; i++) {
    const char c = s[n - 1 - i];
    uint32_t d;
    if (c >= '0' && c <= '9') d = (uint32_t)(c - '0');
    else if (c >= 'a' && c <= 'f') d = (uint32_t)(c - 'a' + 10);
    else return false;
    w[i / 8] |= d << (4 * (i % 8));
  }
  return true;
}

static void print_hex(const uint32_t* w, int words) {
  for (int i = words - 1; i >= 0; i--) printf("%08x", w[i]);
}

int main(int argc, char** argv) {
  FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!in) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<char> line(1 << 16);
  while (fgets(line.data(), (int)line.size(), in)) {
    std::vector<std::string> tok;
    for (char* t = strtok(line.data(), " \t\r\n"); t; t = strtok(nullptr, " \t\r\n")) tok.push_back(t);
    if (tok.empty()) continue;
    if (tok[0] == "plan") {  // plan <n> <ncu> (decimal)
      if (tok.size() != 3) return 3;
      const P384Plan p = verify_p384_plan(atol(tok[1].c_str()), atol(tok[2].c_str()));
      printf("%ld %ld\n", p.threads, p.blocks);
      continue;
    }
    const int op = p384_op_code(tok[0].c_str());
    if (op < 0 || (int)tok.size() - 1 != p384_op_inputs(op)) {
      fprintf(stderr, "bad command: %s\n", tok[0].c_str());
      return 3;
    }
    uint32_t inw[P384_OP_MAX_IN][P384_OP_WORDS] = {}, outw[P384_OP_MAX_OUT][P384_OP_WORDS] = {};
    for (size_t k = 1; k < tok.size(); k++)
      if (!parse_hex(tok[k].c_str(), inw[k - 1])) {
        fprintf(stderr, "bad operand: %s\n", tok[k].c_str());
        return 3;
      }
    p384_op_run(op, inw, outw);
    for (int k = 0; k < p384_op_outputs(op); k++) {
      if (k) printf(" ");
      print_hex(outw[k], P384_OP_WORDS);
    }
    printf("\n");
  }
  if (in != stdin) fclose(in);
  return 0;
}
