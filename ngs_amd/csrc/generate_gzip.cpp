// generate_gzip.cpp -- ngsq_gzip_pipe_* (include/ngsq_generate.h): the `.fastq.gz` output of
// `ngs generate`.  The writer thread of a file writes its text into a pipe as it would into the file; a few threads here
// take pieces off the pipe in turn, compress each into a gzip member of its own (zlib, level 6) and write the members in
// the pieces' order.  Any gzip reader sees the text the plain file would hold.  Host only, no HIP.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ngsq_generate.h"

namespace {

constexpr size_t GZ_PIECE = (size_t)1 << 20;

// one gzip member holding in[0, n) appended to *out; false: zlib failed
bool gzip_member(const uint8_t *in, size_t n, std::vector<uint8_t> *out) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
    out->resize(deflateBound(&z, (uLong)n) + 64);
    z.next_in = const_cast<Bytef *>(in);
    z.avail_in = (uInt)n;
    z.next_out = out->data();
    z.avail_out = (uInt)out->size();
    const int rc = deflate(&z, Z_FINISH);
    const size_t got = out->size() - z.avail_out;
    deflateEnd(&z);
    if (rc != Z_STREAM_END) return false;
    out->resize(got);
    return true;
}

int write_fully(int fd, const uint8_t *p, size_t n) {
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            return errno;
        }
        if (w == 0) return EIO;
        p += w;
        n -= (size_t)w;
    }
    return 0;
}

} // namespace

struct ngsq_gzip_pipe {
    int out_fd = -1, read_fd = -1;
    std::mutex read_mu, write_mu;
    std::condition_variable write_cv;
    uint64_t next_piece = 0, next_write = 0, bytes_in = 0;
    bool eof = false;
    int err = 0; // errno of a failed read or write (EPROTO: zlib): the pipe is drained, nothing more is written
    std::vector<std::thread> th;

    void work() {
        std::vector<uint8_t> in(GZ_PIECE), out;
        for (;;) {
            size_t n = 0;
            uint64_t piece;
            {
                std::lock_guard<std::mutex> g(read_mu); // a piece is read whole by one thread: the pieces' order is the text's
                while (!eof && n < GZ_PIECE) {
                    const ssize_t r = read(read_fd, in.data() + n, GZ_PIECE - n);
                    if (r < 0) {
                        if (errno == EINTR) continue;
                        std::lock_guard<std::mutex> gw(write_mu);
                        if (!err) err = errno;
                        eof = true;
                    } else if (r == 0) {
                        eof = true;
                    } else {
                        n += (size_t)r;
                    }
                }
                if (!n) return;
                piece = next_piece++;
                bytes_in += n;
            }
            const bool ok = gzip_member(in.data(), n, &out);
            std::unique_lock<std::mutex> g(write_mu);
            write_cv.wait(g, [&] { return next_write == piece; });
            if (!ok && !err) err = EPROTO;
            if (!err) err = write_fully(out_fd, out.data(), out.size());
            next_write++;
            write_cv.notify_all();
        }
    }
};

extern "C" {

int ngsq_gzip_pipe_open(int out_fd, int n_threads, ngsq_gzip_pipe **out, int *write_fd) {
    if (out_fd < 0 || !out || !write_fd) return NGSQ_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int fds[2];
    if (pipe2(fds, O_CLOEXEC) != 0) return NGSQ_ERR_INVALID_ARGUMENT;
#ifdef F_SETPIPE_SZ
    (void)fcntl(fds[1], F_SETPIPE_SZ, (int)GZ_PIECE); // (best effort: fewer wake-ups per piece)
#endif
    ngsq_gzip_pipe *p = new ngsq_gzip_pipe();
    p->out_fd = out_fd;
    p->read_fd = fds[0];
    const int nt = n_threads > 0 ? (n_threads > 16 ? 16 : n_threads) : 8;
    for (int t = 0; t < nt; t++) p->th.emplace_back([p] { p->work(); });
    *out = p;
    *write_fd = fds[1];
    return NGSQ_OK;
}

/* 0, or the errno of the first failure */
int ngsq_gzip_pipe_close(ngsq_gzip_pipe *p) {
    if (!p) return 0;
    for (auto &t : p->th) t.join();
    int err = p->err;
    if (!err && !p->bytes_in) { // an empty text is one empty member
        std::vector<uint8_t> out;
        err = gzip_member(nullptr, 0, &out) ? write_fully(p->out_fd, out.data(), out.size()) : EPROTO;
    }
    close(p->read_fd);
    delete p;
    return err;
}

} // extern "C"
