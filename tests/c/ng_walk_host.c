/* ng_walk_host.c — stand-alone host check of the pcapng reader (gopacket_amd/csrc/gpd_pcapng.cpp).
 *
 * Built by tests/test_pcapng.py with gpd_pcapng.cpp (-DGPD_PCAPNG_STANDALONE: no runtime, no
 * HIP) under -fsanitize=address,undefined and run on the CPU only: the reader must not read
 * outside the capture, divide by zero or overflow a signed integer on any input.
 *
 *   ng_walk_host [--cut] [--opts WES] FILE...
 *
 * Every FILE is copied into a heap block of exactly its length (so that the sanitizer sees a
 * read one byte past it), opened with the given options (W want_mixed_linktype, E
 * error_on_mismatching_linktype, S skip_unknown_version, - none) and read to its stop in bounded
 * calls of 7 packets; every packet's bytes are summed, so a packet pointing outside the capture
 * is a sanitizer report.  The interfaces and the section strings are read too.  One line per
 * file: "name packets stop pos checksum".  --cut repeats that for every truncation of the file
 * and prints "name/cut truncations total-packets".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gpd_pcapng.h"

static unsigned long long touch(const uint8_t *buf, uint64_t len, gpd_pcapng_str s) {
  unsigned long long sum = 0;
  if (s.off == UINT64_MAX) return s.len;
  if (s.off + s.len > len) {
    fprintf(stderr, "string outside the capture\n");
    exit(3);
  }
  for (uint32_t i = 0; i < s.len; i++) sum += buf[s.off + i];
  return sum;
}

static int walk(const uint8_t *buf, uint64_t len, const gpd_pcapng_opts *o, uint64_t *n_all, int *stop_out,
                uint64_t *pos, unsigned long long *sum) {
  gpd_pcapng_reader *r = NULL;
  int stop = 0;
  *n_all = 0;
  *sum = 0;
  *pos = 0;
  int rc = gpd_pcapng_open(buf, len, o, &r, &stop);
  if (rc != GPD_OK) {
    if (rc != GPD_ERR_PCAPNG || r != NULL || gpd_pcapng_last_error()[0] == 0) return 2;
    *stop_out = stop;
    return 0;
  }
  uint32_t off[7], cap[7], wire[7], nsec[7], ifx[7], lt[7];
  int64_t sec[7];
  for (;;) {
    uint64_t n = 0;
    rc = gpd_pcapng_index(r, 7, off, cap, wire, sec, nsec, ifx, lt, &n, &stop);
    if (rc != GPD_OK && rc != GPD_ERR_PCAPNG) return 2;
    for (uint64_t i = 0; i < n; i++) {
      if ((uint64_t)off[i] + cap[i] > len || nsec[i] >= 1000000000u) return 2;
      for (uint32_t j = 0; j < cap[i]; j++) *sum += buf[off[i] + j];
      *sum += (unsigned long long)sec[i] + nsec[i] + wire[i] + ifx[i] + lt[i];
    }
    *n_all += n;
    if (stop != GPD_PCAPNG_STOP_LIMIT) break;
  }
  gpd_pcapng_section_info si;
  if (gpd_pcapng_section(r, &si) != GPD_OK) return 2;
  *sum += touch(buf, len, si.hardware) + touch(buf, len, si.os) + touch(buf, len, si.application) +
          touch(buf, len, si.comment);
  for (uint32_t i = 0; i < gpd_pcapng_ninterfaces(r); i++) {
    gpd_pcapng_iface f;
    if (gpd_pcapng_interface(r, i, &f) != GPD_OK) return 2;
    *sum += touch(buf, len, f.name) + touch(buf, len, f.comment) + touch(buf, len, f.description) +
            touch(buf, len, f.filter) + touch(buf, len, f.os) + f.second_mask;
  }
  *pos = gpd_pcapng_pos(r);
  *stop_out = stop;
  gpd_pcapng_close(r);
  return 0;
}

int main(int argc, char **argv) {
  gpd_pcapng_opts o;
  memset(&o, 0, sizeof o);
  o.device_walk = -1;
  int cut = 0;
  for (int a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "--cut")) {
      cut = 1;
      continue;
    }
    if (!strcmp(argv[a], "--opts") && a + 1 < argc) {
      const char *f = argv[++a];
      o.want_mixed_linktype = strchr(f, 'W') != NULL;
      o.error_on_mismatching_linktype = strchr(f, 'E') != NULL;
      o.skip_unknown_version = strchr(f, 'S') != NULL;
      continue;
    }
    FILE *fp = fopen(argv[a], "rb");
    if (!fp) {
      perror(argv[a]);
      return 1;
    }
    fseek(fp, 0, SEEK_END);
    long len = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t *all = malloc(len ? (size_t)len : 1);
    if (fread(all, 1, (size_t)len, fp) != (size_t)len) return 1;
    fclose(fp);
    uint64_t n, pos, total = 0;
    unsigned long long sum;
    int stop = 0;
    if (walk(all, (uint64_t)len, &o, &n, &stop, &pos, &sum)) {
      fprintf(stderr, "%s: reader misbehaved\n", argv[a]);
      return 2;
    }
    printf("%s %llu %d %llu %llu\n", argv[a], (unsigned long long)n, stop, (unsigned long long)pos, sum);
    if (cut) {
      for (long k = 0; k < len; k++) {
        uint8_t *part = malloc(k ? (size_t)k : 1); /* exactly k bytes: a read at [k] is reported */
        memcpy(part, all, (size_t)k);
        if (walk(part, (uint64_t)k, &o, &n, &stop, &pos, &sum)) {
          fprintf(stderr, "%s cut at %ld: reader misbehaved\n", argv[a], k);
          return 2;
        }
        total += n;
        free(part);
      }
      printf("%s/cut %ld %llu\n", argv[a], len, (unsigned long long)total);
    }
    free(all);
  }
  return 0;
}
