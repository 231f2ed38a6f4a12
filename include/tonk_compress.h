/*
    tonk_compress.h -- Tonk's upstream compression step on MI355X.

    Replaces tonk::MessageCompressor (PacketCompression.h:92-140, PacketCompression.cpp:28-118):
    messages of a reliable in-order stream are compressed against the stream's history so that
    the reference's tonk::MessageDecompressor (PacketCompression.cpp:120-216: zstd
    ZSTD_decompressBlock / ZSTD_insertBlock over a 24,000-byte history ring) restores them
    unchanged.  Each compressed message is one zstd compressed block (RFC 8878) built on the GPU
    (tonk_amd/csrc/lz.hip); a message that does not shrink is reported with written = 0 and is
    sent as is (the decompressor then calls InsertUncompressed), exactly the reference contract.
    There is no CPU fallback: without a gfx950 device creation fails.

    The receive side replaces tonk::MessageDecompressor (PacketCompression.h:210-260,
    PacketCompression.cpp:120-216) the same way: tamd_decompressor_* restore zstd compressed
    blocks on the GPU (tonk_amd/csrc/unlz.hip) against the same 24,000-byte history ring, the
    reference compressor's blocks and this library's alike, with no zstd on the host.
*/
#ifndef TONK_COMPRESS_H
#define TONK_COMPRESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* MessageCompressor::Initialize (PacketCompression.cpp:28-61): null when no device is usable. */
void* tamd_compressor_create(unsigned max_compressed_message_bytes);

/* MessageCompressor::Compress (PacketCompression.cpp:70-118): 0 on success with *written = the
   compressed bytes in dest (at most max_compressed_message_bytes), or 0 when the message should be
   sent uncompressed; negative on a device error (the compressor then stays failed, as the
   reference's "compressor has stopped unexpectedly").  bytes must be 1..max. */
int   tamd_compressor_compress(void* c, const uint8_t* data, unsigned bytes, uint8_t* dest, unsigned* written);

void  tamd_compressor_destroy(void* c);

/* The device-resident batch (bench.py --workload compress): n_streams independent compressor
   streams, stream s's messages back to back at dev_data + s * stride (device memory, with at
   least 32 readable bytes after a stream's last message), message k of stream s is
   lens[s * n_msgs + k] bytes (1..max_bytes).  Every stream starts fresh (history
   empty) and applies MessageCompressor's Allocate(max)/Commit ring rule.  Outputs: message
   (s, k) compressed at dev_out + (s * n_msgs + k) * max_bytes, written_host[s * n_msgs + k]
   (0: send uncompressed).  msgs_per_job consecutive messages of a stream share one wave's hash
   table (0: chosen so that the jobs fill the device's wave slots once).  *kernel_ms (optional) = the compression kernel's duration.  Returns 0 or negative. */
int   tamd_compress_batch(const void* dev_data, uint64_t stride, uint32_t n_streams, uint32_t n_msgs,
                          const uint32_t* lens, uint32_t max_bytes, void* dev_out, uint32_t* written_host,
                          uint32_t msgs_per_job, float* kernel_ms);

/* The same batch from host memory: host_data is copied to the device first and the compressed
   messages come back to host_out (n_streams * n_msgs * max_bytes bytes). */
int   tamd_compress_batch_host(const void* host_data, uint64_t stride, uint32_t n_streams, uint32_t n_msgs,
                               const uint32_t* lens, uint32_t max_bytes, void* host_out, uint32_t* written_host,
                               uint32_t msgs_per_job, float* kernel_ms);

/* MessageDecompressor::Initialize (PacketCompression.cpp:136-152): null when no device is usable
   or the size is 0 or above the 24,000-byte history. */
void* tamd_decompressor_create(unsigned max_compressed_message_bytes);

/* MessageDecompressor::InsertUncompressed (PacketCompression.cpp:162-176): a message that was
   sent as is enters the history.  Does not wait for the device: the bytes are queued and ride, in
   order, with the decompressor's next tamd_decompressor_decompress (the queue is flushed on its
   own once it holds a few times the history's size).  A message outside 1..max is ignored. */
void  tamd_decompressor_insert_uncompressed(void* d, const uint8_t* data, unsigned bytes);

/* MessageDecompressor::Decompress (PacketCompression.cpp:178-208): restores one compressed block
   into dest; 0 on success with *restored = the message's bytes.  Negative when the block is
   malformed (-17 and below: the block reader's reason, tonk_amd/csrc/unlz.h status - 16), when
   dest_cap is smaller than the message (-4; nothing is written) or on a device error; the
   decompressor then stays failed, as the reference's connection closes. */
int   tamd_decompressor_decompress(void* d, const uint8_t* block, unsigned bytes, uint8_t* dest, unsigned dest_cap,
                                   unsigned* restored);

void  tamd_decompressor_destroy(void* d);

/* The device-resident batch: n_streams independent fresh streams of n_msgs messages each, one
   wave per stream.  Message (s, k), i = s * n_msgs + k, occupies the slot dev_in + i * max_bytes
   with in_bytes[i] bytes: a compressed block when is_block[i] is set, else the message itself
   (it goes through the InsertUncompressed path and is copied to its output slot unchanged).  At
   least 32 readable bytes follow the last input slot.  The input (those 32 bytes included) and the
   output must not overlap: blocks are read in place while output slots are written.  Outputs: the
   restored message at dev_out +
   i * max_bytes, restored_host[i] = its bytes, status_host[i] = 0 or the reason the block was
   rejected (negative, unlz.h); after a rejected block the stream's remaining messages are not
   decoded (status -13) and their output slots are left untouched.  tamd_compress_batch chains
   into it: dev_out and written feed it directly with in_bytes[i] = written[i] (lens[i] when
   written[i] is 0) and is_block[i] = written[i] > 0, once the caller has copied the messages sent
   uncompressed into their slots.  *kernel_ms (optional) = the kernel's duration.  Returns 0 or
   negative (-5: the kernel wrote outside its streams' memory). */
int   tamd_decompress_batch(const void* dev_in, uint32_t n_streams, uint32_t n_msgs, const uint32_t* in_bytes,
                            const uint8_t* is_block, uint32_t max_bytes, void* dev_out, uint32_t* restored_host,
                            int32_t* status_host, float* kernel_ms);

/* The same batch from host memory (n_streams * n_msgs * max_bytes bytes each way; output slots a
   message does not fill keep what host_out held). */
int   tamd_decompress_batch_host(const void* host_in, uint32_t n_streams, uint32_t n_msgs, const uint32_t* in_bytes,
                                 const uint8_t* is_block, uint32_t max_bytes, void* host_out, uint32_t* restored_host,
                                 int32_t* status_host, float* kernel_ms);

#ifdef __cplusplus
}
#endif

#endif
