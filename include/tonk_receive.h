/*
    tonk_receive.h -- the front of Tonk's receive path for a tick's datagrams in the caller's own
    device memory: footer read, nonce expansion, anti-replay, tag check, decipher.

    One handle owns, per connection (stream), the cipher key and the anti-replay state of Tonk's
    security::StrikeRegister: a 4096-bit window, its base, its rotation and the largest accepted
    nonce.  The caller hands over the datagrams as they came off the wire -- datagram i of a call
    at base + i * pitch, any alignment -- and every one goes through what
    SessionIncoming::ProcessDatagram does before it walks the messages, with the reference's
    results for the same datagrams in the same per-connection order: the datagrams of one stream
    are processed in list order (the expansion of a datagram sees the largest nonce accepted so
    far, those of this very call included); streams are independent of each other and of their
    places in the list.  Only result lists cross to the host.

    A connected datagram of `bytes` bytes ends in its footer (TonkineseProtocol.h):

        sequence bytes (0..3) | nonce bytes (0..3) | handshake (12, flag 0x40) | timestamp (3) |
        flags (1) | tag (2)

    flags: 0x80 connection datagram, 0x40 handshake, 0x20 SeqComp, 0x10 OnlyFEC, bits 3..2 nonce
    bytes, bits 1..0 sequence bytes.

    Per-datagram result codes (rc[i]), in the reference's order of checks:

        1  invalid: bytes below 6 + handshake + nonce bytes + sequence bytes as its own flags byte
           gives them, bytes above max_datagram_bytes, or flag 0x80 clear.  Nothing is read
           further, nothing changes.
        3  duplicate: IsDuplicate(nonce) after the expansion (no nonce bytes: LargestSequence + 1,
           else CounterExpand against LargestSequence).  The tag is not looked at; the datagram
           and the state stay as they were.
        2  bad tag: the datagram and the state stay byte for byte as they were.
        0  the nonce was accepted (StrikeRegister::Accept) and the first message_bytes = bytes -
           footer bytes were deciphered.
        4  as 0, but the datagram is Tonk's "Ignored re-ordered" (sequence bytes > 0, fewer than
           the nonce bytes, and LargestSequence + 1 > nonce + 1 after the accept): the caller must
           not process its messages.

    result[i] is filled for every rc except 1 (all zero there).

    A function's own return value is 0, or negative when the call as a whole was refused and
    nothing was done: -1 bad handle or null pointer, -2 a stream id >= n_streams, -3 a pitch
    smaller than the call's largest `bytes`, -4 device error (sticky: every later call returns it;
    tamd_recv_error() has the text).

    Calls are synchronous and serialised per handle by the library.  receive writes only
    [0, message_bytes) of the datagrams with rc 0 or 4 and nothing else in the caller's memory,
    whatever the pitch and alignment.

    Not part of this interface, and left with the caller: the expansion of the reliable sequence
    number (partial_seq and seq_bytes are returned; it needs the decoder's next expected packet
    number), time synchronisation (timestamp24 is returned), the handshake hook (a datagram with
    the handshake flag is processed as when Tonk's handler says "continue"),
    DisableSequenceNumberCompress as the reaction to rc 2 and 3, key exchange, asynchronous calls.
*/
#ifndef TONK_RECEIVE_H
#define TONK_RECEIVE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamd_recv_params {
    uint32_t device, n_streams;
    uint32_t max_datagram_bytes;   /* 1..65535 */
} tamd_recv_params;

typedef struct tamd_recv_result {
    uint64_t nonce;            /* the expanded nonce */
    uint32_t message_bytes;    /* bytes - ConnectedFooterBytes: the message section */
    uint32_t timestamp24;
    uint32_t partial_seq;      /* the low seq_bytes bytes of the reliable sequence number */
    uint8_t  flags, seq_bytes, nonce_bytes, handshake_bytes;
} tamd_recv_result;

#define TAMD_RECV_STATE_WORDS 67u  /* what tamd_recv_state returns: largest, base, rotation, 64 window words */

/* NULL with a message in err when the parameters are bad ("bad parameters") or no gfx950 device is
   usable ("no HIP device ...").  There is no CPU fallback. */
void* tamd_recv_create(const tamd_recv_params*, char* err, size_t err_len);
void  tamd_recv_destroy(void*);
const char* tamd_recv_error(void*);

/* SimpleCipher::Initialize for one stream, as tamd_seal_set_key: a fresh stream's key is 0; the
   key takes effect with the next call. */
int tamd_recv_set_key(void*, uint32_t stream, uint64_t key);
/* StrikeRegister::Reset(base) for one stream.  A fresh stream is Reset(0). */
int tamd_recv_reset(void*, uint32_t stream, uint64_t base);

/* Datagram i belongs to stream[i] and is bytes[i] long at dev_datagrams + i * pitch. */
int tamd_recv_receive(void*, uint32_t n, const uint32_t* stream, const uint32_t* bytes, void* dev_datagrams, uint64_t pitch,
                      int32_t* rc, tamd_recv_result* result);

/* LargestSequence + 1 of the streams named, for the acknowledgements the caller sends: from a host
   mirror kept from the results, without a device call. */
int tamd_recv_next_expected(void*, uint32_t n, const uint32_t* stream, uint64_t* out);
/* Tests and diagnostics: the stream's state read back from the device into
   out[0 .. TAMD_RECV_STATE_WORDS): LargestSequence, WindowBase, WindowBitRotation, the window. */
int tamd_recv_state(void*, uint32_t stream, uint64_t* out);

/* Measurement (tools/recv_time.py): out[0..3] = milliseconds the predict (footer parse and nonce
   guesses), tag, resolve and decipher kernels took on the device since the last call (HIP events
   around each launch, only recorded after tamd_recv_set_timing(h, 1)), out[4..7] the launches of
   each, out[8] the datagrams whose tag had to be computed again in the resolve step because the
   guessed nonce was wrong. */
void tamd_recv_set_timing(void*, int on);
void tamd_recv_kernel_ms(void*, double* out, unsigned n);

#ifdef __cplusplus
}
#endif

#endif
