/*
    tonk_datagram.h -- batched building and parsing of Tonk datagrams in the caller's own device
    memory: the step between the codecs of tonk_batch.h and the cipher and tag of tonk_seal.h.

    The sender's side (tamd_dgram_build) writes message frames and footers where Tonk's
    sendQueuedDatagram and PostRecovery do; the receiver's side (tamd_dgram_parse) walks the frame
    headers of a deciphered message section as ProcessDatagram does, or as resumeProcessing and
    onCompressed walk a recovered original or a decompressed payload.  The bytes are Tonk's, so
    either end of a connection may be a stock Tonk peer.  The handle holds no per-connection state.

    A connected datagram as built (F = its footer fields):

        messages         each u16_le(type << 11 | bytes) || body, in list order; or, in an OnlyFEC
                         datagram, one recovery packet as tamd_batch_encode returned it, no header
        seq_bytes        (0..3) low bytes of the sequence number, little-endian
        nonce_bytes      (0..3) low bytes of the nonce
        12 bytes         the handshake, when attached
        3 bytes          the 24-bit timestamp, little-endian
        1 byte           flags: 0x80 | handshake 0x40 | seqcomp 0x20 | onlyfec 0x10 | nonce_bytes << 2 | seq_bytes
        2 bytes          zeros, where tamd_seal_seal puts the tag

    Item i of a call is at base + i * pitch, at any alignment; lists and results are host arrays.
    A function's own return value is 0, or negative when the call as a whole was refused and
    nothing was done: -1 bad handle or null pointer, -2 (build) a datagram index that is >= n or
    smaller than the one before it, -3 a pitch too small (build: below the 6 bytes of the shortest
    datagram; parse: offset[i] + bytes[i] > pitch for a section of valid length), -4 device error
    (sticky: every later call returns it; tamd_dgram_error() has the text).

    Calls are synchronous and serialised per handle by the library.  build writes only
    [0, out_bytes[i]) of a slot and parse writes nothing on the device: slots next to an item are
    never written, whatever the pitch and alignment.

    What stays with the caller: the choice of how many sequence and nonce bytes to send and their
    expansion back to whole numbers on the receiving side (Tonk's writeNonce, its sequence
    compression and Counter::ExpandFromTruncated); the check "Reliable data sent with no sequence
    number", which is a test of the flags byte against reliable_bytes; anti-replay; the delivery
    of the parsed messages; decompression of Compressed bodies (tonk_compress_batch.h restores them
    where the parse found them); handshake contents; Tonk's queueing of messages into datagrams;
    asynchronous calls.  OnlyFEC datagrams are not parsed: the caller sees the flag in
    tamd_seal_footers' bytes and hands the message section to tamd_batch_decoder_add_recovery.
*/
#ifndef TONK_DATAGRAM_H
#define TONK_DATAGRAM_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamd_dgram_params {
    uint32_t device;
    uint32_t max_datagram_bytes;   /* 8..65535 */
} tamd_dgram_params;

#define TAMD_DGRAM_HANDSHAKE_BYTES 12u
#define TAMD_DGRAM_TYPE_RAW 255u       /* build: the headerless body of an OnlyFEC datagram */
#define TAMD_DGRAM_SEQCOMP 0x20u       /* flag_bits taken by build (kSeqCompMask, kOnlyFECMask) */
#define TAMD_DGRAM_ONLYFEC 0x10u

/* NULL with a message in err when the parameters are bad ("bad parameters") or no gfx950 device is
   usable ("no HIP device ...").  There is no CPU fallback. */
void* tamd_dgram_create(const tamd_dgram_params*, char* err, size_t err_len);
void  tamd_dgram_destroy(void*);
const char* tamd_dgram_error(void*);

/* sender side: n datagrams from m messages.  Message j goes into datagram dgram[j] (non-decreasing
   over j) with type[j] 0..31, bytes[j] 0..2047 and its body at the device address src[j] (any
   alignment; 0: a body of zeros, the Padding frame's).  Datagram i gets the low seq_bytes[i] bytes
   of seq[i], the low nonce_bytes[i] bytes of nonce[i] (both 0..3), the 12 bytes at
   handshake + 12 * i when has_handshake[i] (handshake may be null: none in this call; has_handshake
   is then not read), timestamp24[i], and of flag_bits[i] the SeqComp and OnlyFEC bits.  An OnlyFEC
   datagram takes exactly one message of type TAMD_DGRAM_TYPE_RAW (any length that fits) and no
   sequence bytes.  Datagram i is written at dev_out + i * pitch.

   Host results per datagram: out_bytes and message_bytes (what tamd_seal_seal takes);
   reliable_offset and reliable_bytes, the span from the header of the first message of type >= 5
   to the end of the last (0, 0 without one): what goes to tamd_batch_encoder_add_at; rc 0, or 1
   for invalid input, with nothing of the slot written: a type above 31; bytes above 2047; seq_bytes
   or nonce_bytes above 3; a total above max_datagram_bytes or pitch; reliable messages without
   seq_bytes; a message of type < 5 behind a reliable one, unless it is Padding (type 4), which may
   follow reliable data and ends the reliable span before it (only Padding may then follow); an
   OnlyFEC datagram of another shape, or a raw message outside one. */
int tamd_dgram_build(void*, uint32_t n, uint32_t m, const uint32_t* dgram, const uint32_t* type, const uint32_t* bytes,
                     const uint64_t* src, const uint32_t* seq, const uint32_t* seq_bytes, const uint32_t* nonce,
                     const uint32_t* nonce_bytes, const uint8_t* handshake, const uint8_t* has_handshake,
                     const uint32_t* timestamp24, const uint32_t* flag_bits, void* dev_out, uint64_t pitch,
                     uint32_t* out_bytes, uint32_t* message_bytes, uint32_t* reliable_offset, uint32_t* reliable_bytes,
                     int32_t* rc);

/* receiver side: n message sections, section i bytes[i] long at dev + i * pitch + offset[i] (a null
   offset: all 0).  mode 0 applies ProcessDatagram's rules, mode 1 those of resumeProcessing and
   onCompressed (no AckAck rule).  Host results per section: status 0 ok, 1 not walked (bytes[i]
   above max_datagram_bytes), 2 "Truncated message" (a header announces more than remains), 3
   "Invalid frame" (one byte is left over), 4 "Invalid ackack" (mode 0: an AckAck whose length is
   not 3); the walk stops at the first error.  n_messages: the frames walked before the end or
   the error, also above cap.  reliable_offset, reliable_bytes: from the first reliable frame's
   header to the last reliable frame's end, over the frames walked (0, 0 without one).
   table[i * cap + k], written for k < min(n_messages[i], cap): type << 27 | bytes << 16 |
   payload_offset, the offset relative to the section's start.  table may be null when cap is 0. */
int tamd_dgram_parse(void*, uint32_t n, const uint32_t* bytes, const uint32_t* offset, const void* dev, uint64_t pitch,
                     uint32_t mode, uint32_t cap, uint32_t* status, uint32_t* n_messages, uint32_t* reliable_offset,
                     uint32_t* reliable_bytes, uint32_t* table);

/* Measurement (tools/dgram_time.py): out[0..1] = milliseconds the build and the parse kernel took
   on the device since the last call (HIP events around each launch, only recorded after
   tamd_dgram_set_timing(h, 1)), out[2..3] the launches of each. */
void tamd_dgram_set_timing(void*, int on);
void tamd_dgram_kernel_ms(void*, double* out, unsigned n);

#ifdef __cplusplus
}
#endif

#endif
