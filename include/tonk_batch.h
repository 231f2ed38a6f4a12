/*
    tonk_batch.h -- batched encoders and decoders over the caller's own device packets.

    One handle owns n_streams independent connections, each with an encoder and a decoder (use
    either side or both).  The caller hands over a tick's worth of packets of all connections in
    device memory -- packet i of a call at base + i * pitch, any alignment -- and gets recovery
    packets, or recovered originals, back in device memory the same way.  Every stream's results
    are those of the siamese.h codec given the same calls in the same per-stream order; result
    codes per packet or stream are the siamese.h values:

        0 Success  1 InvalidInput  2 NeedMoreData  3 MaxPacketsReached  4 DuplicateData  5 Disabled

    A function's own return value is 0, or negative when the call as a whole was refused and
    nothing was done: -1 bad handle or null pointer, -2 a stream id >= n_streams, -3 a pitch
    smaller than the call's largest packet, -4 device error (sticky: every later call returns it;
    tamd_batch_error() has the text).

    Calls are synchronous: when one returns, the caller's input buffers may be reused and its
    output buffers are complete.  Added originals are copied into device rows the codec owns.
    The control planes run on the calling thread; calls on one handle are serialised by the
    library.

    Not part of this interface: worker pools, level pipelining across calls,
    siamese_encoder_retransmit, siamese_encoder_remove_before, and zero-copy access to the
    codec's device rows.
*/
#ifndef TONK_BATCH_H
#define TONK_BATCH_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamd_batch_params {
    uint32_t device, n_streams;
    uint32_t max_packet_bytes;   /* payload bytes of the largest original, 1..65535 */
    uint64_t arena_bytes;        /* device arena, split evenly over the streams */
} tamd_batch_params;

/* A recovery packet is at most this much longer than the largest original (length header and
   footer): the pitch of tamd_batch_encode's output must hold max_packet_bytes + this. */
#define TAMD_BATCH_RECOVERY_OVERHEAD 11u

/* NULL with a message in err when the parameters are bad or no gfx950 device is usable
   ("no HIP device ..."). */
void* tamd_batch_create(const tamd_batch_params*, char* err, size_t err_len);
void  tamd_batch_destroy(void*);
const char* tamd_batch_error(void*);

/* sender side: packet i belongs to stream[i], is len[i] bytes at dev_payloads + i * pitch; packets
   of one stream are added in list order.  rc[i], packet_num[i] per packet (host arrays).  A packet
   with len 0 or above max_packet_bytes gets rc 1 and is skipped. */
int tamd_batch_encoder_add(void*, uint32_t n, const uint32_t* stream, const uint32_t* len,
                           const void* dev_payloads, uint64_t pitch, uint32_t* packet_num, int32_t* rc);
/* the same with packet i at dev_payloads + i * pitch + offset[i] (a null offset: all 0, the call
   above): a span inside a larger slot, such as the reliable messages of a datagram
   (tonk_datagram.h).  -3 when offset[i] + len[i] > pitch for a packet of valid length. */
int tamd_batch_encoder_add_at(void*, uint32_t n, const uint32_t* stream, const uint32_t* len, const uint32_t* offset,
                              const void* dev_payloads, uint64_t pitch, uint32_t* packet_num, int32_t* rc);
/* one recovery packet per list entry (a stream may appear several times), in list order: packet i
   (data || footer, exactly what siamese_encode returns) at dev_out + i * pitch, bytes[i] long
   (0 unless rc[i] is 0).  pitch >= max_packet_bytes + TAMD_BATCH_RECOVERY_OVERHEAD. */
int tamd_batch_encode(void*, uint32_t n, const uint32_t* stream, void* dev_out, uint64_t pitch,
                      uint32_t* bytes, int32_t* rc);
/* siamese_encoder_ack of one stream (host bytes); returns its result code, or negative as above */
int tamd_batch_encoder_ack(void*, uint32_t stream, const uint8_t* data, uint32_t bytes, uint32_t* next_expected);

/* receiver side */
int tamd_batch_decoder_add_original(void*, uint32_t n, const uint32_t* stream, const uint32_t* packet_num,
                                    const uint32_t* len, const void* dev_payloads, uint64_t pitch, int32_t* rc);
/* the same with packet i at dev_payloads + i * pitch + offset[i], as tamd_batch_encoder_add_at */
int tamd_batch_decoder_add_original_at(void*, uint32_t n, const uint32_t* stream, const uint32_t* packet_num,
                                       const uint32_t* len, const uint32_t* offset, const void* dev_payloads,
                                       uint64_t pitch, int32_t* rc);
/* packet i (data || footer) is bytes[i] long at dev_packets + i * pitch; 0 bytes, or more than
   max_packet_bytes + TAMD_BATCH_RECOVERY_OVERHEAD, gets rc 1 */
int tamd_batch_decoder_add_recovery(void*, uint32_t n, const uint32_t* stream, const uint32_t* bytes,
                                    const void* dev_packets, uint64_t pitch, int32_t* rc);
/* every listed stream: is_ready, and when it is, decode.  stream_rc[k] per listed stream (NeedMoreData
   when not ready).  Recovered originals, in list order and increasing packet number inside a stream:
   payload j at dev_out + j * pitch, out_stream[j], out_packet_num[j], out_bytes[j]; *n_out of them,
   at most cap (a stream whose packets would not fit is not decoded in this call: NeedMoreData,
   nothing lost).  Slot bytes past out_bytes[j] are not written.  A stream with a recovered packet
   whose length header is malformed, announces 0 bytes or more than the packet can hold (or more
   than pitch) is disabled (stream_rc 5) and none of its packets of the call are returned.
   pitch >= max_packet_bytes. */
int tamd_batch_decode(void*, uint32_t n, const uint32_t* stream, void* dev_out, uint64_t pitch, uint32_t cap,
                      uint32_t* out_stream, uint32_t* out_packet_num, uint32_t* out_bytes, uint32_t* n_out,
                      int32_t* stream_rc);
/* siamese_decoder_ack of one stream (host buffer); returns its result code, or negative as above */
int tamd_batch_decoder_ack(void*, uint32_t stream, uint8_t* buffer, uint32_t limit, uint32_t* used);

/* Measurement (tools/batch_time.py): out[0..3] = milliseconds the framing, unframing and tail
   kernels and the codec programs took on the device since the last call (HIP events around each
   launch; the events are only recorded after tamd_batch_set_timing(h, 1)), out[4..7] the launches
   of each, out[8..9] the bytes the framing and unframing kernels moved. */
void tamd_batch_set_timing(void*, int on);
void tamd_batch_kernel_ms(void*, double* out, unsigned n);

#ifdef __cplusplus
}
#endif

#endif
