// arx_feeder.cpp -- C ABI of the FASTQ feeder (feeder.h); host code only.
#include <stdio.h>
#include "feeder.h"

extern "C" {

int arx_feeder_open(const char *r1_path, const char *r2_path, arx_feeder **out, char *msg, int32_t msg_cap)
{
	*out = nullptr;
	arx::Feeder *f = nullptr;
	try {
		f = new arx::Feeder();
		if (!f->open(r1_path, r2_path)) {
			if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", f->error.c_str());
			delete f;
			return ARX_E_IO;
		}
	} catch (const std::exception &e) {
		if (msg && msg_cap > 0) snprintf(msg, (size_t)msg_cap, "%s", e.what());
		delete f;
		return ARX_E_IO;
	}
	*out = (arx_feeder *)(arx::FeederBase *)f;
	return ARX_OK;
}

int arx_feeder_next(arx_feeder *h, int64_t target_pairs, arx_super_batch *out)
{
	try {
		return ((arx::FeederBase *)h)->next(target_pairs, out);
	} catch (const std::exception &) {
		return ARX_E_IO;
	}
}

void arx_feeder_close(arx_feeder *h)
{
	try { delete (arx::FeederBase *)h; } catch (...) {}
}

int arx_feeder_device_reads(arx_feeder *h, const uint8_t **d_bases, const int32_t **d_lens, int64_t *n_bases)
{
	return h ? ((arx::FeederBase *)h)->device_reads(d_bases, d_lens, n_bases) : ARX_E_ARG;
}

int arx_feeder_stats(arx_feeder *h, int64_t *stats) { return h && stats ? ((arx::FeederBase *)h)->stats(stats) : ARX_E_ARG; }

int arx_feeder_gunzip_stats(arx_feeder *h, int64_t *stats) { return h && stats ? ((arx::FeederBase *)h)->gunzip_stats(stats) : ARX_E_ARG; }

}
