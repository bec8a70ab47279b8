// mel_spikes_kernel.inc -- the text of the one-launch mel kernel, included once per form: mel.hip defines the kernel's name
// (LSM_MEL_KERNEL), its parameters (LSM_MEL_PARAMS) and the encoder call that ends it (LSM_MEL_ENCODE).  One text, two kernels -- and not one device
// function called by two: behind a call the unmasked kernel compiled to other code (profiles/spec_mask.txt).
// MASK (SPEC.md 1.13): the finishing workgroup's encoder masks the normalised values with `m`; nothing else differs.
__global__ __launch_bounds__(256) void LSM_MEL_KERNEL(LSM_MEL_PARAMS)
{
    // four waves, a point buffer each (dynamic: 68 KB); the finishing workgroup reuses them as the raster stage
    extern __shared__ __attribute__((aligned(16))) unsigned char mel_lds[];
    double2 *buf = reinterpret_cast<double2 *>(mel_lds);
    float *red = reinterpret_cast<float *>(mel_lds + 4 * sizeof(double2) * ZPAD);       // 4 floats
    int &last = *reinterpret_cast<int *>(red + 4);
    const int b = blockIdx.y, tid = threadIdx.x, w = tid >> 6;
    // A workgroup takes `frames_per_wg` consecutive frames, its four waves one frame each at a time: the release fence below
    // writes the XCD's dirty L2 lines back (the eight L2s are not coherent with each other), which costs about a microsecond,
    // so it is paid once per group of frames, not once per frame (one frame per workgroup: 2.4 instead of 0.3 ms per
    // 200 clips, profiles/r04_mel_one_launch_ab.txt).
    const int t0 = (int)blockIdx.x * a.frames_per_wg;
    const int t1 = min(t0 + a.frames_per_wg, a.mel.n_frames);
    for (int t = t0 + w; t < t1; t += 4) {
        mel_clip_frame(a.mel, buf + w * ZPAD, b, t);
        mel_wave_fence();                       // the wave's LDS buffers are free again
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");      // my power values are visible device-wide before my count is
    __syncthreads();
    if (tid == 0) {
        const unsigned int prev = atomicAdd(a.counters + b, 1u);
        last = prev == gridDim.x - 1u;
        if (last) a.counters[b] = 0u;           // every workgroup of the clip has counted: reset for the next launch
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // the other workgroups' values, not whatever this CU may have cached
    const int n = a.mel.n_mels * a.mel.n_frames;
    float *db = const_cast<float *>(a.sp.db) + (size_t)b * n;
    power_to_db_body(a.mel.power_out + (size_t)b * n, db, n, a.amin, a.top_db, red);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // dB values written by other threads of this workgroup
    __syncthreads();
    LSM_MEL_ENCODE;                             // lsm_fe::spec_to_spikes_body on (a.sp, b, mel_lds), masked with `m` or not
}
