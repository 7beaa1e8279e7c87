// k_rows.inc — the rows of a video stream's per-track states, included by k_tracks.hip in front of every state.  A stream keeps its
// points, the track table, the depths, the templates, the keyframe with its map and the zones' rejects as arrays with one row per
// track; every step each of them drops the rows whose status is 0, moves the kept rows up IN ORDER and appends fresh rows for the
// re-detected corners.  All of them do it through the functions below, so row i of one state and row i of another are the same track.
//
// The walk: one workgroup of 256 threads per stream takes the rows in chunks of 256, thread tid the row i0 + tid: it reads the row,
// asks rows_place for its destination, stores it there and calls rows_next.  A chunk is read completely before any of its rows is
// written (the second barrier of rows_place), and a row only moves to a position <= its own, so an array can be compacted in place: no
// row is overwritten before it has been read.  Plain stores and no atomics, so a second launch on the same inputs gives the same bits.
struct row_walk { int wave[4]; int base; };                      // LDS: the kept rows per wave of this chunk, the kept rows of the chunks before

__device__ __forceinline__ void rows_begin(row_walk &w) { if (threadIdx.x == 0) w.base = 0; __syncthreads(); }

// The destination of this thread's row among the kept rows (meaningful where keep)
__device__ __forceinline__ int rows_place(row_walk &w, bool keep)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) w.wave[wave] = __popcll(bal);
    __syncthreads();
    int off = w.base;
    for (int q = 0; q < wave; ++q) off += w.wave[q];
    const int pos = off + __popcll(bal & ((1ull << lane) - 1));
    __syncthreads();                                            // every thread has read its row of this chunk: safe to overwrite
    return pos;
}

// The chunk is stored: on to the next one.  Behind the last chunk w.base is the number of kept rows.
__device__ __forceinline__ void rows_next(row_walk &w) { if (threadIdx.x == 0) w.base += w.wave[0] + w.wave[1] + w.wave[2] + w.wave[3]; __syncthreads(); }

// The fresh rows behind the `kept` ones: the re-detected corners (new_counts NULL: none), as far as max_total and the stride go
__device__ __forceinline__ int rows_extra(const int *__restrict__ new_counts, int b, int max_total, int stride, int kept)
{
    return new_counts ? max(0, min(min(new_counts[b], max_total - kept), stride - kept)) : 0;
}

// Does a launch over the streams b0 .. b0 + batch - 1 touch stream b?  limit != NULL: only those with a budget, as k_replace_tracks
__device__ __forceinline__ bool rows_stream_on(int b, int b0, int batch, const int *__restrict__ limit)
{
    return b < b0 + batch && (!limit || limit[b] > 0);
}
