/*
    tonk_compress_batch.h -- batched, stateful compression and decompression of Tonk's reliable
    messages in the caller's own device memory.

    One handle owns the compression history of n_streams connections: per stream the 64 KB ring of
    tonk_compress.h's MessageCompressor drop-in (sender side) and the state and 24,000-byte ring of
    its MessageDecompressor (receiver side).  The caller hands over a tick's messages of any subset
    of the connections where they lie in device memory -- message i of a call at device address
    src[i], any alignment -- and gets blocks, or restored messages, at dev_out + i * out_pitch.
    The history stays on the device from call to call; no message crosses to the host.

    Sender: tamd_cbatch_compress.  written[i] == 0 means "send as is", exactly
    MessageCompressor::Compress's contract: the caller frames the original bytes at src[i] and no
    copy of them is made.  Otherwise the block of written[i] bytes is at dev_out + i * out_pitch.
    Items of one stream are that stream's next messages in array order; a stream may have no, one
    or many items in a call.  For every stream the written values and the blocks are those that
    tamd_compressor_compress (a MessageCompressor of the same maximum) returns when fed the
    stream's messages in the same order, however they were spread over calls and whatever the
    other streams did, with one exception that only a handle created with `abut` has: see below.  tonk::MessageDecompressor restores every block.

    Receiver: tamd_cbatch_decompress.  Item i is a compressed block (is_block[i] != 0), restored to
    dev_out + i * out_pitch, or a message that was sent as is, which enters its stream's history
    only (MessageDecompressor::InsertUncompressed): nothing is written for it, restored[i] =
    bytes[i].  status[i] is 0 or the block reader's negative reason:
        -1 the block ends inside a header or a section     -8  sequence bit stream
        -2 literals section header                         -9  more literals used than the block has
        -3 Huffman tree description                        -10 an offset reaches beyond the history
        -4 a Huffman stream is not consumed exactly        -11 more restored than the maximum
        -5 treeless / repeat with no earlier table         -12 the block restores nothing
        -6 sequences section header                        -13 an earlier item of the stream failed
        -7 FSE table description                           -14 bytes[i] is 0 or above the maximum
    After a rejected item the stream stays failed: its later items in this and in later calls get
    -13 and touch nothing, until tamd_cbatch_reset.  Other streams are unaffected.  The restored
    bytes are those tonk::MessageDecompressor returns.
    Blocks are read in place.  The caller guarantees 32 readable bytes after every block (a body
    inside a datagram buffer has them whenever the buffer is 32 bytes longer than its largest
    datagram) and that no input of a call overlaps the call's output.

    `abut` (a field of the parameters) lets a call compress several messages of one stream in one
    pass over the stream's ring, as many as the ring holds beside their windows (about 40 KB), where
    a handle without it takes one message per stream and pass.  A call whose busiest stream has k
    messages is then a few launches, not 2 k.  The compression kernel lets up to four bytes behind a
    message's end into the hash keys of its last four positions; with messages abutting in a pass
    those are the head of the next message, not what the ring held before, so the last sequence of
    a block may differ from the per-message interface's (a match of 4..7 bytes found or missed at
    the message's very end).  Every block is still one that MessageDecompressor restores.

    A function's own return value is 0, or negative when the call as a whole was refused and
    nothing was done: -1 bad handle, null pointer, a side the handle was not created with, in
    compress a bytes[i] outside 1..max_message_bytes or a call whose output n * out_pitch exceeds
    4 GiB (the kernel's output offsets are 32-bit; split the call); -2 a stream id >= n_streams;
    -3 out_pitch < max_message_bytes; -4 device error (sticky: every later call returns it;
    tamd_cbatch_error() has the text; a write that left the handle's stream memory is reported
    this way too).  Calls are synchronous and serialised per handle by the library.

    The functions are in libtonk_amd_cbatch.so, built beside libtonk_amd.so.

    Not part of this interface: framing (tonk_datagram.h; the parse there returns where the
    Compressed bodies are), the cipher (tonk_seal.h), FEC (tonk_batch.h), asynchronous calls.
*/
#ifndef TONK_COMPRESS_BATCH_H
#define TONK_COMPRESS_BATCH_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TAMD_CBATCH_COMPRESS 1u    /* sides: the sender's state, a 64 KB ring and its mirror per stream */
#define TAMD_CBATCH_DECOMPRESS 2u  /* sides: the receiver's state, about 35 KB per stream */

typedef struct tamd_cbatch_params {
    uint32_t device, n_streams;
    uint32_t max_message_bytes;  /* 1..24000, as tamd_compressor_create */
    uint32_t sides;              /* TAMD_CBATCH_*: only what is asked for is allocated */
    uint32_t abut;               /* 0, or 1: several messages of a stream per pass (see above) */
} tamd_cbatch_params;

/* NULL with a message in err when the parameters are bad ("bad parameters") or no gfx950 device is
   usable ("no HIP device ...").  There is no CPU fallback. */
void* tamd_cbatch_create(const tamd_cbatch_params*, char* err, size_t err_len);
void  tamd_cbatch_destroy(void*);
const char* tamd_cbatch_error(void*);

int tamd_cbatch_compress(void*, uint32_t n, const uint32_t* stream, const uint64_t* src, const uint32_t* bytes,
                         void* dev_out, uint64_t out_pitch, uint32_t* written);
int tamd_cbatch_decompress(void*, uint32_t n, const uint32_t* stream, const uint64_t* src, const uint32_t* bytes,
                           const uint8_t* is_block, void* dev_out, uint64_t out_pitch, uint32_t* restored, int32_t* status);

/* The named streams return to the fresh state on the sides named (TAMD_CBATCH_COMPRESS,
   TAMD_CBATCH_DECOMPRESS): empty history, not failed -- a slot reused by a new connection. */
int tamd_cbatch_reset(void*, uint32_t n, const uint32_t* stream, uint32_t sides);

/* Measurement (tools/cbatch_time.py): out[0..3] = milliseconds the placement, compression and
   decompression kernels took on the device since the last call (HIP events around each launch,
   only recorded after tamd_cbatch_set_timing(h, 1)) and one spare, out[4..7] the launches of each. */
void tamd_cbatch_set_timing(void*, int on);
void tamd_cbatch_kernel_ms(void*, double* out, unsigned n);

#ifdef __cplusplus
}
#endif

#endif
