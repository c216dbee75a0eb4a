/* bpf_host.c — the host half of include/gpd_bpf.h from a plain C program: the validator and
 * gpd_bpf_run_host over a file of cases, every result compared with the value the file expects
 * (the checker's, tests/bpf_ref.py).  Built from gopacket_amd/csrc/gpd_bpf_host.cpp alone with
 * -DGPD_BPF_STANDALONE and -fsanitize=address,undefined (tests/test_bpf.py); each program and
 * each packet gets a heap block of exactly its size, so a read beyond either is reported.
 *
 *   bpf_host <cases file>
 *
 * The file, all numbers decimal:
 *   prog <ninsn> <valid 0|1> <bad index> <npackets>
 *   <code> <jt> <jf> <k>                        ninsn lines
 *   <wirelen> <expected> <caplen> <hex | ->     npackets lines (valid programs only)
 * Prints "bpf_host ok <programs> <runs>" and returns 0, or the first mismatch and 1.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpd_bpf.h"

static int hexval(int c) {
  return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: bpf_host <cases file>\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  unsigned long programs = 0, runs = 0;
  unsigned ninsn, valid, bad, npk;
  static char hex[1 << 16];
  while (fscanf(f, " prog %u %u %u %u", &ninsn, &valid, &bad, &npk) == 4) {
    gpd_bpf_insn *prog = (gpd_bpf_insn *)malloc(ninsn ? ninsn * sizeof *prog : 1);
    for (unsigned i = 0; i < ninsn; i++) {
      unsigned code, jt, jf, k;
      if (fscanf(f, "%u %u %u %u", &code, &jt, &jf, &k) != 4) {
        fprintf(stderr, "program %lu: bad instruction line\n", programs);
        return 2;
      }
      prog[i].code = (uint16_t)code;
      prog[i].jt = (uint8_t)jt;
      prog[i].jf = (uint8_t)jf;
      prog[i].k = k;
    }
    const int rc = gpd_bpf_validate(prog, ninsn);
    if ((rc == GPD_OK) != (valid != 0)) {
      printf("program %lu: validate gave %d (%s), expected %s\n", programs, rc, gpd_last_error_string(),
             valid ? "valid" : "invalid");
      return 1;
    }
    if (!valid) {
      char want[32];
      snprintf(want, sizeof want, "instruction %u ", bad);
      if (ninsn >= 1 && ninsn <= GPD_BPF_MAX_INSNS && !strstr(gpd_last_error_string(), want)) {
        printf("program %lu: error text \"%s\" does not name instruction %u\n", programs, gpd_last_error_string(), bad);
        return 1;
      }
      /* a refused program never runs: 0, whatever the packet */
      const uint8_t one = 1;
      if (gpd_bpf_run_host(prog, ninsn, &one, 1, 1) != 0) {
        printf("program %lu: refused, but gpd_bpf_run_host ran it\n", programs);
        return 1;
      }
    }
    for (unsigned p = 0; p < npk; p++) {
      unsigned wirelen, expect, caplen;
      if (fscanf(f, "%u %u %u %65535s", &wirelen, &expect, &caplen, hex) != 4) {
        fprintf(stderr, "program %lu: bad packet line\n", programs);
        return 2;
      }
      uint8_t *data = (uint8_t *)malloc(caplen ? caplen : 1);
      if (caplen) {
        if (strlen(hex) != 2u * caplen) {
          fprintf(stderr, "program %lu packet %u: %zu hex digits for %u bytes\n", programs, p, strlen(hex), caplen);
          return 2;
        }
        for (unsigned b = 0; b < caplen; b++) data[b] = (uint8_t)(hexval(hex[2 * b]) << 4 | hexval(hex[2 * b + 1]));
      }
      /* caplen 0: a pointer to a block the interpreter must not touch */
      const uint32_t got = gpd_bpf_run_host(prog, ninsn, caplen ? data : data + 1, caplen, wirelen);
      if (got != expect) {
        printf("program %lu packet %u: returned %u, expected %u\n", programs, p, got, expect);
        return 1;
      }
      free(data);
      runs++;
    }
    free(prog);
    programs++;
  }
  fclose(f);
  printf("bpf_host ok %lu %lu\n", programs, runs);
  return 0;
}
