// What xcg_pipe.cpp shares with xcg_codec.cpp (nobody else includes this): the
// two halves of xcg_pipe_encoder_consume_many.  encode_step runs the encode()
// calls of every pipe's frames in one GPU batch and makes the pipes' state
// changes -- <HELLO> sent, the frames' reference maps, <EOS> sent
// (xcodec/xcodec_pipe_pair.cc:549-642); emit_wire writes one pipe's wire from
// what the step left.  The pair layer calls one after the other; the codec
// layer, with a compressor, keeps the encodings on the device (`on_device`)
// and builds the wire there (xcg_wire_plan.h).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/xcgpu.h"

namespace xcg {
namespace pipe {

struct Encoded {
  // per pipe of the call
  std::vector<uint8_t> hello, eos;     // this call sends <HELLO> / <EOS>
  std::vector<uint32_t> first;         // n + 1: pipe k's frames are [first[k], first[k + 1])
  // per frame: its encoding at enc_off[f], enc_len[f] bytes
  std::vector<uint64_t> enc_off, enc_len;
  std::vector<uint8_t> enc;            // the encodings on the host (empty with on_device)
  const uint8_t* d_enc = nullptr;      // on_device: in the encoder context's staging, valid until the
                                       // context's next host-convenience call
};

// XCG_EINVAL if xcg_pipe_encoder_consume_many would refuse the call; nothing changes.
int encode_check(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n);
// (after encode_check) XCG_OK, or an engine failure with no pipe changed.  Every pipe's outputs are cleared.
int encode_step(xcg_pipe* const* pipes, const uint8_t* const* data, const uint64_t* len, uint32_t n, bool on_device,
                Encoded* e);
// Pipe k's wire into its to_peer.
void emit_wire(xcg_pipe* p, const Encoded& e, uint32_t k);

const uint8_t* uuid_of(const xcg_pipe* p);      // the 36 bytes its <HELLO> carries
bool sent_eos(const xcg_pipe* p);               // encoder_sent_eos_
xcg_ctx* encoder_ctx(const xcg_pipe* p);
void outputs(const xcg_pipe* p, xcg_pipe_out* o);   // what its last call produced

}  // namespace pipe
}  // namespace xcg
