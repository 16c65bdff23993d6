// mcrx_scan.cc -- "what is on the air?": a band scan on the channel monitor of libmcrx_hip.so (include/mcrx_hip.h, mcrx_hip_monitor_*).
// Reads IQ from the synthetic UHD stand-in like the other host programs ($MCRX_IQ_FILE, $MCRX_IQ_PACKET), pushes it through a
// multichannel receiver with the monitor on and prints, per interval, a table
//     channel  level[dB]  peak[dB]  occupied
// and one text row of the wideband spectrum: the N * nfft bins of all channels in frequency order, folded (mean power) to the
// terminal width, ten grey levels from an offset in steps of so many dB.  One mcrx_hip_monitor_read(reset = 1) per interval: the
// rows tile the stream like the rows of a waterfall.  The receiver keeps decoding meanwhile; frames are counted, not shown.
//   -n channels (8)   -M subcarriers (64)   -C cyclic prefix (16)   -T taper (4)    -w bins per channel: 16 .. 256 (64)
//   -W window: 0 rectangular, 1 Hann (default), 2 Hamming       -i intervals (4)    -p packets per interval (64)
//   -c columns of the spectrum row (64)     -o offset [dB] of the lowest grey level (default: 45 dB below the interval's largest bin)
//   -s step [dB] per grey level (5)         -d a channel is occupied within this many dB of the strongest (20)
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <unistd.h>
#include "uhd/usrp/multi_usrp.hpp"
#include "mcrx_hip.h"

static double db(double v) { return 10.0 * log10(v > 1e-30 ? v : 1e-30); }

int main(int argc, char **argv)
{
    unsigned N = 8, M = 64, cp = 16, taper = 4, nfft = 64, window = 1, intervals = 4, packets = 64, cols = 64;
    double offset = NAN, step = 5.0, occ_db = 20.0;
    int o;
    while ((o = getopt(argc, argv, "n:M:C:T:w:W:i:p:c:o:s:d:h")) != -1) {
        switch (o) {
        case 'n': N = (unsigned)atoi(optarg); break;
        case 'M': M = (unsigned)atoi(optarg); break;
        case 'C': cp = (unsigned)atoi(optarg); break;
        case 'T': taper = (unsigned)atoi(optarg); break;
        case 'w': nfft = (unsigned)atoi(optarg); break;
        case 'W': window = (unsigned)atoi(optarg); break;
        case 'i': intervals = (unsigned)atoi(optarg); break;
        case 'p': packets = (unsigned)atoi(optarg); break;
        case 'c': cols = (unsigned)atoi(optarg); break;
        case 'o': offset = atof(optarg); break;
        case 's': step = atof(optarg); break;
        case 'd': occ_db = atof(optarg); break;
        default:
            fprintf(stderr, "usage: %s [-n channels] [-M subcarriers] [-C cp] [-T taper] [-w nfft] [-W window] [-i intervals] [-p packets] [-c columns] [-o offset_dB] [-s step_dB] [-d occupied_dB]\n", argv[0]);
            return o == 'h' ? 0 : 1;
        }
    }
    if (cols < 1 || step <= 0.0 || intervals < 1 || packets < 1) { fprintf(stderr, "error: %s, columns, step, intervals and packets must be positive\n", argv[0]); return 1; }
    mcrx_hip_t rx = NULL;
    if (mcrx_hip_create(&rx, N, M, cp, taper, NULL, NULL) != MCRX_OK) { fprintf(stderr, "error: %s\n", mcrx_hip_last_error()); return 1; }
    mcrx_hip_monitor_config mc;
    mc.struct_size = sizeof(mc); mc.nfft = nfft; mc.window = window;
    if (mcrx_hip_monitor_enable(rx, &mc) != MCRX_OK) { fprintf(stderr, "error: %s\n", mcrx_hip_last_error()); mcrx_hip_destroy(rx); return 1; }

    uhd::device_addr_t addr;
    uhd::usrp::multi_usrp::sptr usrp = uhd::usrp::multi_usrp::make(addr);
    uhd::device::sptr dev = usrp->get_device();
    std::vector<std::complex<float> > buf(dev->get_max_recv_samps_per_packet());
    uhd::rx_metadata_t md;

    std::vector<double> level(N), psd((size_t)N * nfft), row(cols);
    std::vector<float> peak(N);
    static const char grey[] = " .:-=+*#%@";
    unsigned long frames_total = 0;
    for (unsigned it = 0; it < intervals; it++) {
        for (unsigned p = 0; p < packets; p++) {
            const size_t n = dev->recv(buf.data(), buf.size(), md, uhd::io_type_t::COMPLEX_FLOAT32, uhd::device::RECV_MODE_ONE_PACKET);
            const int rc = mcrx_hip_execute_host(rx, reinterpret_cast<const float *>(buf.data()), n);
            if (rc != MCRX_OK && rc != MCRX_EOVERFLOW) { fprintf(stderr, "error: %s\n", mcrx_hip_last_error()); mcrx_hip_destroy(rx); return 1; }
        }
        mcrx_hip_flush(rx);
        uint64_t fr = 0, ok = 0, bytes = 0, nseg = 0, nsamp = 0;
        mcrx_hip_drain_count(rx, &fr, &ok, &bytes);
        frames_total += (unsigned long)fr;
        if (mcrx_hip_monitor_read(rx, level.data(), peak.data(), psd.data(), &nseg, &nsamp, 1) != MCRX_OK) { fprintf(stderr, "error: %s\n", mcrx_hip_last_error()); mcrx_hip_destroy(rx); return 1; }
        double top = 0.0, top_bin = 0.0;
        for (unsigned c = 0; c < N; c++) if (level[c] > top) top = level[c];
        for (double v : psd) if (v > top_bin) top_bin = v;
        printf("interval %u: %llu samples and %llu segments per channel, %llu frames decoded\n", it, (unsigned long long)nsamp, (unsigned long long)nseg, (unsigned long long)fr);
        printf("channel  level[dB]  peak[dB]  occupied\n");
        for (unsigned c = 0; c < N; c++)
            printf("%7u  %9.2f  %8.2f  %s\n", c, db(level[c]), db(peak[c]), (nsamp && db(level[c]) > db(top) - occ_db) ? "yes" : "no");
        // wideband order: channel by channel, signed bins -nfft/2+1 .. nfft/2 (omega(c, k')), folded to `cols` columns
        const size_t nb = (size_t)N * nfft;
        std::vector<unsigned> cnt(cols, 0);
        for (auto &v : row) v = 0.0;
        for (size_t i = 0; i < nb; i++) {
            const unsigned c = (unsigned)(i / nfft);
            const int kp = (int)(i % nfft) - (int)nfft / 2 + 1;
            const size_t col = i * cols / nb;
            row[col] += psd[(size_t)c * nfft + (size_t)((kp + (int)nfft) % (int)nfft)]; cnt[col]++;
        }
        const double off = std::isnan(offset) ? db(top_bin) - 45.0 : offset;
        printf("|");
        for (unsigned j = 0; j < cols; j++) {
            const double v = cnt[j] ? db(row[j] / cnt[j]) : -300.0;
            int g = (int)floor((v - off) / step);
            putchar(grey[g < 0 ? 0 : (g > 9 ? 9 : g)]);
        }
        printf("|\n");
    }
    printf("%lu frames decoded in all\n", frames_total);
    mcrx_hip_destroy(rx);
    return 0;
}
