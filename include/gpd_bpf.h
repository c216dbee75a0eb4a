/*
 * gpd_bpf.h — C-ABI of the filter step: a classic BPF program run over a device batch, one
 * packet per lane, giving the `keep` bytes gpd_pcap_write and gpd_batch_select read
 * (gpd_pcapwrite.h).  capture -> filter -> select -> decode -> flow table / pcap out, in HBM.
 *
 * The reference hands BPF programs to libpcap and to the kernel: it holds the instruction
 * format, the program-length rule and the call shape of Matches, and forwards the rest.  The
 * machine itself is libpcap's bpf_filter; its rules are restated below and in
 * gopacket_amd/csrc/gpd_bpf_vm.h, which the device kernel and gpd_bpf_run_host share.
 *
 * Reference interfaces each entry point replaces (paths relative to google/gopacket):
 *   gpd_bpf_insn       pcap.BPFInstruction{Code, Jt, Jf, K}                 pcap/pcap.go:113-119
 *   gpd_bpf_validate   the length rule of SetBPFInstructionFilter            pcap/pcap.go:36,504-511
 *                      (the instruction rules are libpcap's bpf_validate, which pcap_setfilter runs)
 *   gpd_bpf_create     pcap.NewBPFInstructionFilter                          pcap/pcap.go:553-573
 *                      (also what Handle.SetBPFInstructionFilter pcap/pcap.go:465-514,
 *                       afpacket.TPacket.SetBPF afpacket/afpacket.go:265-266 and
 *                       pcapgo.EthernetHandle.SetBPF pcapgo/capture.go:184-186 install)
 *   gpd_bpf_filter     the loop `keep[i] = f.Matches(ci[i], data[i])`        pcap/pcap_unix.go:342-352
 *   gpd_bpf_run_host   (*BPF).Matches for one host packet, as its return value
 *
 * The machine.  A, X and M[0..15] are u32 and start at 0; execution starts at instruction 0; all
 * arithmetic is mod 2^32; comparisons are unsigned.  buflen is the packet's capture length
 * (Matches: len(data)), wirelen is CaptureInfo.Length.  "fails" = the program ends and returns 0.
 *   LD W/H/B ABS   A = big-endian 4/2/1 bytes at k     fails when k > buflen or size > buflen - k
 *                                                      (B: k >= buflen)
 *   LD W/H IND     A = big-endian 4/2 bytes at X + k   fails when k > buflen or X > buflen - k or
 *                                                      size > buflen - (X + k)
 *   LD B IND       A = the byte at X + k               fails when k >= buflen or X >= buflen - k
 *   LDX B MSH      X = (byte at k & 0xf) << 2          fails when k >= buflen
 *   LD/LDX IMM, MEM, LEN   k, M[k], wirelen            never fail
 *   ST, STX        M[k] = A, M[k] = X
 *   ALU ADD SUB MUL DIV MOD AND OR XOR LSH RSH with K or X, and NEG (A = 0 - A)
 *                  DIV or MOD by X == 0 fails; LSH or RSH by X >= 32 gives A = 0
 *   JA             pc += k
 *   JEQ JGT JGE JSET with K or X (JSET: A & src)       pc += cond ? jt : jf
 *   RET K, RET A   the program returns k, A
 *   TAX, TXA
 * Opcode numbers are those of linux/bpf_common.h and linux/filter.h.
 *
 * Validation (once, by gpd_bpf_validate and gpd_bpf_create): 1 <= len <= 4096; every code is one
 * of the forms above; M indices < 16; DIV|K and MOD|K with k == 0 and LSH|K and RSH|K with
 * k >= 32 are refused; every jump target (i + 1 + k, i + 1 + jt, i + 1 + jf, without a wrap) is
 * < len; the last instruction is a RET.  Jumps only go forward, so a run ends within len steps.
 * A refused program is GPD_ERR_INVALID, and gpd_last_error_string() names the instruction index
 * and the reason.
 *
 * Where this differs from the reference and from libpcap, and why:
 *  - M starts at zero.  libpcap leaves it indeterminate; a filter that reads a cell before it
 *    writes one gets 0 here, on the host and on the device alike.
 *  - A packet of capture length 0: (*BPF).Matches panics on it (`&data[0]`, pcap_unix.go:348).
 *    Here every packet load of such a packet fails, and loads of k, M and wirelen work as ever.
 *  - The Linux ancillary offsets (k >= 0xfffff000: SKF_AD_*) get no special case.  They are out
 *    of range and fail, as pcap_offline_filter does without auxiliary data.
 *  - LSH / RSH by X >= 32 give A = 0 (libpcap leaves C's undefined shift to the compiler), and
 *    the validator refuses a constant shift of 32 or more.
 *  - RET X, NEG with the X source bit and LDX with a size other than the forms above are refused
 *    (libpcap's validator lets some of them through and then ignores the bit).
 *  - A descriptor that reaches past data_len is read as gpd_decode reads it: offset and caplen
 *    clamped to the buffer; the clamped caplen is buflen.
 *  - Compiling a filter expression (pcap.CompileBPFFilter, NewBPF) is libpcap's compiler and is
 *    not here: programs come as instructions, e.g. pasted from `tcpdump -dd`.
 */
#ifndef GPD_BPF_H_
#define GPD_BPF_H_
#include "gpd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GPD_BPF_MAX_INSNS 4096u /* pcap.MaxBpfInstructions (pcap/pcap.go:36) */

typedef struct gpd_bpf_insn { uint16_t code; uint8_t jt, jf; uint32_t k; } gpd_bpf_insn; /* pcap.BPFInstruction */
typedef struct gpd_bpf gpd_bpf;

/* The validation rules above; host only, no device.  GPD_OK or GPD_ERR_INVALID. */
int gpd_bpf_validate(const gpd_bpf_insn *prog, uint32_t len);

/* NewBPFInstructionFilter: validates the program and uploads it to the context's device.  The
 * filter holds no reference to `prog` afterwards.  It must be destroyed before its context. */
int gpd_bpf_create(gpd_ctx *ctx, const gpd_bpf_insn *prog, uint32_t len, gpd_bpf **out);
void gpd_bpf_destroy(gpd_bpf *f);

/* The loop `keep[i] = f.Matches(ci[i], data[i])` over a device batch.
 *   in       the batch (device pointers, the usual batch contract: any layout)
 *   wirelen  u32[n] device, CaptureInfo.Length; NULL means Length = the capture length
 *   keep     u8[n] device: 1 when the program returns nonzero for packet i, else 0
 *   ret      u32[n] device, or NULL: the program's return value (the snap length libpcap
 *            would apply)
 * Queued on `stream`; the call does not synchronise and allocates nothing.  It writes exactly n
 * entries of keep (and of ret), and issues no load from `data` outside
 * [0, round_up(data_len, 16)).  n == 0 is a no-op.  One filter may serve any number of calls and
 * streams at once: a call changes nothing in it. */
int gpd_bpf_filter(gpd_bpf *f, const gpd_batch *in, const uint32_t *wirelen, uint8_t *keep, uint32_t *ret,
                   void *stream);

/* One host packet through the same interpreter compiled for the host: the value whose `!= 0` is
 * (*BPF).Matches.  A program the validator refuses returns 0 (gpd_last_error_string() says why). */
uint32_t gpd_bpf_run_host(const gpd_bpf_insn *prog, uint32_t len, const uint8_t *data, uint32_t caplen,
                          uint32_t wirelen);

#ifdef __cplusplus
}
#endif
#endif /* GPD_BPF_H_ */
