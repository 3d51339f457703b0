// csrc/jpegdec.hip <-> csrc/capi.hip: the arguments of the JPEG decode kernels, the workspace layout and the launcher.
#pragma once

struct JpegArgs {
    const unsigned char* data; const int* frames; const int* tables; const int* geom; const int* lengths;      // the JpegClips members
    unsigned char* out; int* status;
    short* coef; int* starts; int* owner; int* rowmap; unsigned char* samp;                                       // the workspace's parts
    long data_bytes;
    int rows, sets, N, T, H, W, lanes, blocks_max;
};

struct JpegLayout { long coef, starts, owner, rowmap, samp, total; };                                            // byte offsets, each a multiple of 256

// the sync entropy mode (jpeg_entropy_sync_kernel): threads of a workgroup, LDS bytes per subsequence, the most subsequences of a frame
#define JP_SYNC_THREADS 128
#define JP_SYNC_SUB_LDS 32
#define JP_SYNC_MAX_SUBS 1536

void jpeg_workspace_layout(int rows, long slots, int lanes, int blocks_max, JpegLayout* l);
int jpeg_decode_launch(JpegArgs a, void* ws, void* stream);
int jpeg_decode_sync_launch(JpegArgs a, void* ws, void* stream, int sub_bytes, int max_subs);
