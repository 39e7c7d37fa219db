// TEST INFRASTRUCTURE ONLY: a C driver around wanproxy's XCodecPipePair, built
// two ways by oracle/Makefile from the reference's own sources:
//   _ref/libppref.so     xcodec/xcodec_pipe_pair.cc over the reference's
//                        XCodecEncoder / XCodecDecoder / XCodecCache
//   _ref/libppdropin.so  the same xcodec_pipe_pair.cc over the integration/
//                        adapters (XCodecEncoder / XCodecDecoder on libxcgpu.so)
// Both link the reference's PipeProducer, Buffer, Mutex and log code.  The two
// PipeProducerWrappers of a pair are driven by direct consume() calls under the
// pair's own mutex; what they produce()d is read out of PipeProducer's
// output_buffer_ (the build passes -fno-access-control, as zpipe_driver.cc's
// `#define private public` does for the zlib pipes).  No event system.
//
// THE ONE STAND-IN: UUID::decode and UUID::generate are defined here.  The
// reference's common/uuid/uuid_libuuid.cc needs libuuid's header, which this
// image does not have.  decode() takes the 36-byte string form and accepts
// exactly 8-4-4-4-12 hex digits; every comparing test sends well-formed UUIDs,
// so no result rests on that accept rule.  Everything else is the reference.
//
// One guard besides: the codecs' caches are HeldMemoryCache, an
// XCodecMemoryCache whose replace() keeps one more reference on the new
// segment.  XCodecMemoryCache::replace stores its entry by CacheEntry's implicit
// copy assignment (xcodec/xcodec_cache.h:246-269, :333-336), which takes no
// reference; after name reuse in a <LEARN> (xcodec_pipe_pair.cc:322-329) nothing
// else holds the segment, the pipe pair's own unref() deletes it and the cache
// keeps a dangling pointer -- the next lookup of that hash reads freed memory.
// The guard changes no decision the reference makes (integration/
// xcodec_decoder_xcgpu.cc does the same for its host mirror); it leaks one
// 2 KiB segment per name reuse.
#include <stdint.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include <common/buffer.h>
#include <common/uuid/uuid.h>
#include <common/thread/mutex.h>
#include <event/event_callback.h>
#include <io/pipe/pipe.h>
#include <io/pipe/pipe_pair.h>
#include <io/pipe/pipe_producer.h>
#include <xcodec/xcodec.h>
#include <xcodec/xcodec_cache.h>
#include <xcodec/xcodec_decoder.h>
#include <xcodec/xcodec_encoder.h>
#include <xcodec/xcodec_pipe_pair.h>

#ifdef XCGPU_DROPIN
#include "../integration/xcgpu_binding.h"
#define RELEASE_CACHE(c) xcgpu_binding::forget(c)
#else
#define RELEASE_CACHE(c) do { } while (0)
#endif

bool UUID::decode(Buffer *buf)
{
	if (buf->length() < UUID_SIZE)
		return (false);
	uint8_t s[UUID_SIZE];
	buf->moveout(s, UUID_SIZE);
	string_ = std::string((const char *)s, UUID_SIZE);
	for (unsigned i = 0; i < UUID_SIZE; i++) {
		const uint8_t c = s[i];
		if (i == 8 || i == 13 || i == 18 || i == 23) {
			if (c != '-')
				return (false);
		} else if (!((c >= '0' && c <= '9') || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F'))) {
			return (false);
		}
	}
	return (true);
}

void UUID::generate(void)
{
	string_ = "00000000-0000-4000-8000-000000000000";
}

namespace {

class HeldMemoryCache : public XCodecMemoryCache {
public:
	HeldMemoryCache(const UUID& uuid, size_t limit_bytes) : XCodecMemoryCache(uuid, limit_bytes) { }

	XCodecCache *connect(const UUID& uuid)
	{
		return new HeldMemoryCache(uuid, memory_cache_limit_ * XCODEC_SEGMENT_LENGTH);
	}

	void replace(const uint64_t& hash, BufferSegment *seg)
	{
		XCodecMemoryCache::replace(hash, seg);
		seg->ref();
	}
};

struct Codec {
	XCodecCache *cache;
	XCodec *codec;
};

struct Pair {
	XCodecPipePair *pp;
	std::vector<uint8_t> to_peer, to_local;
};

void take(PipeProducer *p, std::vector<uint8_t>& out)
{
	const size_t n = p->output_buffer_.length();
	out.resize(n);
	if (n) {
		p->output_buffer_.copyout(&out[0], n);
		p->output_buffer_.clear();
	}
}

}  // namespace

extern "C" {

// What one consume produced.  The pointers stay valid until the pair's next
// consume.  The four flags say what the call itself raised: produce_eos on the
// encoder pipe (the peer-facing side is finished: <EOS_ACK> both ways) and on
// the decoder pipe (the local side has all its data), produce_error on each.
struct pp_out {
	const uint8_t *to_peer;
	uint64_t to_peer_len;
	const uint8_t *to_local;
	uint64_t to_local_len;
	int32_t encoder_eos, decoder_eos, encoder_error, decoder_error;
};

// XCodec over XCodecMemoryCache(uuid) (limit_bytes 0) or (uuid, limit_bytes).
void *pp_codec_new(const char *uuid36, uint64_t limit_bytes)
{
	UUID uuid;
	uuid.string_ = uuid36;
	if (uuid.string_.length() != UUID_SIZE)
		return NULL;
	Codec *c = new Codec;
	c->cache = new HeldMemoryCache(uuid, (size_t)limit_bytes);
	c->codec = new XCodec(c->cache);
	return c;
}

void pp_codec_free(void *h)
{
	Codec *c = (Codec *)h;
	delete c->codec;
	RELEASE_CACHE(c->cache);
	delete c->cache;
	delete c;
}

// Entries of a codec's own (encoder) cache.
uint64_t pp_codec_cache_size(void *h)
{
	XCodecMemoryCache *m = dynamic_cast<XCodecMemoryCache *>(((Codec *)h)->cache);
	return m ? (uint64_t)m->segment_hash_map_.size() : ~(uint64_t)0;
}

void *pp_pair_new(void *codec)
{
	Pair *p = new Pair;
	p->pp = new XCodecPipePair("/pipe_driver", ((Codec *)codec)->codec, XCodecPipePairTypeClient);
	return p;
}

void pp_pair_free(void *h)
{
	Pair *p = (Pair *)h;
	delete p->pp;
	delete p;
}

// One encoder_consume (which 0) or decoder_consume (which 1) of in[0..n), under
// the pair's mutex; n 0 is the empty Buffer (EOS / connection closed).  A pair
// whose pipe has produced an error takes no more input, as PipeProducer::input.
void pp_consume(void *h, int which, const uint8_t *in, uint64_t n, pp_out *o)
{
	Pair *p = (Pair *)h;
	XCodecPipePair *pp = p->pp;
	PipeProducer *ep = pp->encoder_pipe_, *dp = pp->decoder_pipe_;
	PipeProducer *tgt = which == 0 ? ep : dp;
	const bool eeos = ep->output_eos_, deos = dp->output_eos_, eerr = ep->error_, derr = dp->error_;
	Buffer b;
	if (n)
		b.append(in, n);
	if (!tgt->error_) {
		ScopedLock _(&pp->mtx_);
		if (which == 0)
			pp->encoder_consume(&b);
		else
			pp->decoder_consume(&b);
	}
	take(ep, p->to_peer);
	take(dp, p->to_local);
	o->to_peer = p->to_peer.empty() ? NULL : &p->to_peer[0];
	o->to_peer_len = p->to_peer.size();
	o->to_local = p->to_local.empty() ? NULL : &p->to_local[0];
	o->to_local_len = p->to_local.size();
	o->encoder_eos = ep->output_eos_ && !eeos;
	o->decoder_eos = dp->output_eos_ && !deos;
	o->encoder_error = ep->error_ && !eerr;
	o->decoder_error = (dp->error_ && !derr) || (which == 1 && derr);
}

// encoder_reference_frames_.size(): frames the peer has not <ADVANCE>d past.
uint64_t pp_pending_frames(void *h)
{
	return ((Pair *)h)->pp->encoder_reference_frames_.size();
}

// Entries of the connected decoder cache (XCodecCache::connect at <HELLO>);
// ~0 before <HELLO>.
uint64_t pp_decoder_cache_size(void *h)
{
	XCodecMemoryCache *m = dynamic_cast<XCodecMemoryCache *>(((Pair *)h)->pp->decoder_cache_);
	return m ? (uint64_t)m->segment_hash_map_.size() : ~(uint64_t)0;
}

// XCodecCache::connect's registry holds every connected cache for the life of
// the process.  Between conversations (no pair alive) the harness empties it,
// so that a UUID used again connects a fresh cache.
void pp_registry_clear(void)
{
	std::map<UUID, XCodecCache *>::iterator it;
	for (it = XCodecCache::cache_map.begin(); it != XCodecCache::cache_map.end(); ++it) {
		RELEASE_CACHE(it->second);
		delete it->second;
	}
	XCodecCache::cache_map.clear();
}

}  // extern "C"
