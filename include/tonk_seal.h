/*
    tonk_seal.h -- batched seal and open of Tonk datagrams in the caller's own device memory.

    One handle owns the keys of n_streams connections.  The caller hands over a tick's worth of
    datagrams of all connections in device memory -- datagram i of a call at base + i * pitch, any
    alignment -- and they are ciphered and tagged, or tag-checked and deciphered, in place.  The
    bytes are those of Tonk's security::SimpleCipher (Cipher, Tag, TagInt) under the same key and
    nonce, so either end of a connection may be a stock Tonk peer.

    A connected datagram of `bytes` bytes (T = bytes - 6):

        [0, message_bytes)   messages: ciphered and tagged
        [message_bytes, T)   handshake, nonce and sequence footers: tagged, not ciphered
        [T, T + 3)           24-bit timestamp, little-endian      \  not covered by the hash; mixed
        [T + 3]              flags                                /  into the tag through TagInt
        [T + 4, T + 6)       tag = Tag(data, T, nonce) ^ TagInt(timestamp << 8 | flags), little-endian

    tamd_seal_seal reads the timestamp and the flags from the datagram: the caller writes them
    BEFORE the call.  (Tonk writes the timestamp last, after its Tag(); here it has to be in place
    when the tag is made.)

    Per-datagram result codes (rc[i]): 0 done; 1 invalid (bytes < 6, bytes > max_datagram_bytes or
    message_bytes > bytes - 6), nothing of the datagram touched; 2 (open only) the tag does not
    match, the datagram is left byte for byte as it was.

    A function's own return value is 0, or negative when the call as a whole was refused and
    nothing was done: -1 bad handle or null pointer, -2 a stream id >= n_streams, -3 a pitch
    smaller than the call's largest `bytes`, -4 device error (sticky: every later call returns it;
    tamd_seal_error() has the text).

    Calls are synchronous and serialised per handle by the library.  seal and open write only
    [0, message_bytes) of a datagram, seal also the tag's two bytes; cipher writes only [0, bytes).
    Slots next to a datagram are never written, whatever the pitch and alignment.

    Not part of this interface: anti-replay (Tonk's StrikeRegister: the caller rejects a repeated
    nonce before or after open), nonce compression and reconstruction, handshakes and key
    exchange, asynchronous calls.
*/
#ifndef TONK_SEAL_H
#define TONK_SEAL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamd_seal_params {
    uint32_t device, n_streams;
    uint32_t max_datagram_bytes;   /* 1..65535 */
} tamd_seal_params;

#define TAMD_SEAL_FOOTER_BYTES 24u  /* what tamd_seal_footers returns per datagram (Tonk's kMaxOverheadBytes) */

/* NULL with a message in err when the parameters are bad ("bad parameters") or no gfx950 device is
   usable ("no HIP device ...").  There is no CPU fallback. */
void* tamd_seal_create(const tamd_seal_params*, char* err, size_t err_len);
void  tamd_seal_destroy(void*);
const char* tamd_seal_error(void*);

/* SimpleCipher::Initialize / Tonk's ChangeEncryptionKey for one stream.  A fresh stream's key is 0
   (no cipher; tags are still made and checked).  The key takes effect with the next call. */
int tamd_seal_set_key(void*, uint32_t stream, uint64_t key);

/* sender side: datagram i belongs to stream[i], is bytes[i] long at dev_datagrams + i * pitch with
   nonce[i]; its first message_bytes[i] bytes are ciphered, then its tag is written. */
int tamd_seal_seal(void*, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                   const uint32_t* message_bytes, void* dev_datagrams, uint64_t pitch, int32_t* rc);
/* receiver side: the tag is recomputed over the bytes as received; on a match the first
   message_bytes[i] bytes are deciphered. */
int tamd_seal_open(void*, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                   const uint32_t* message_bytes, void* dev_datagrams, uint64_t pitch, int32_t* rc);

/* The two primitives alone, for other layouts (handshake datagrams): Cipher over bytes[i] bytes in
   place; plain Tag() values of bytes[i] bytes into a host array.  bytes[i] = 0 is valid; an entry
   above max_datagram_bytes is skipped (not ciphered; tag 0). */
int tamd_seal_cipher(void*, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                     void* dev_data, uint64_t pitch);
int tamd_seal_tag(void*, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                  const void* dev_data, uint64_t pitch, uint16_t* tag);

/* The last min(bytes[i], 24) bytes of each datagram at footers + i * 24 (host), right-aligned and
   zero-filled in front: the receiver reads the flags byte there (footers[i * 24 + 21]) to rebuild
   the nonce and message_bytes before it calls tamd_seal_open. */
int tamd_seal_footers(void*, uint32_t n, const uint32_t* bytes, const void* dev_datagrams, uint64_t pitch,
                      uint8_t* footers);

/* Measurement (tools/seal_time.py): out[0..1] = milliseconds the seal/open/cipher/tag kernel and
   the footer kernel took on the device since the last call (HIP events around each launch, only
   recorded after tamd_seal_set_timing(h, 1)), out[2..3] the launches of each. */
void tamd_seal_set_timing(void*, int on);
void tamd_seal_kernel_ms(void*, double* out, unsigned n);

#ifdef __cplusplus
}
#endif

#endif
