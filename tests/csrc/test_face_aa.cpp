// test_face_aa.cpp -- antialiased face batches through the class header: RetinaFace::detectFaceBatch with spec.antialias set, then
// RetinaFace::detectFaceBatchGated with the same spec and a NULL gate (which must return the same tensor bytes); reads a raw BGR
// frame, runs it as a batch of {frame, empty, frame}, writes what the calls returned for tests/test_face_aa_gpu.py to compare with
// tests/face_aa_ref.py.
//   usage: test_face_aa <model_dir> <stem> <net_h> <net_w> <frame.raw> <rows> <cols> <threshold> <crop> <format> <rgb> <capacity>
//                       <max_faces> <antialias> <aa_max> <out.bin>
//   out.bin: int32 n | int32 truncated | (n + 1) int32 offsets | per image: int32 k, k x 15 float | int32 stride |
//            n x stride rf_face_quality | int32 faces | faces x 6 double | the tensor bytes
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "RetinaFace.h"

int main(int argc, char **argv) {
    if (argc != 17) { fprintf(stderr, "usage: see the head of this file\n"); return 2; }
    string model = argv[1];
    rf_options o = {};
    o.struct_size = sizeof(o);
    o.model_stem = argv[2];
    o.net_h = atoi(argv[3]); o.net_w = atoi(argv[4]);
    const int rows = atoi(argv[6]), cols = atoi(argv[7]);
    rf_face_batch_spec spec = {};
    spec.struct_size = sizeof(spec);
    spec.crop_size = atoi(argv[9]); spec.format = atoi(argv[10]); spec.rgb = atoi(argv[11]); spec.capacity = atoi(argv[12]);
    spec.max_faces = atoi(argv[13]);
    spec.antialias = atoi(argv[14]); spec.aa_max = atoi(argv[15]);
    std::vector<unsigned char> px((size_t)rows * cols * 3);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(px.data(), 1, px.size(), f) != px.size()) { fprintf(stderr, "cannot read %s\n", argv[5]); return 2; }
    fclose(f);
    try {
        RetinaFace det(model, o);
        cv::Mat img(rows, cols, CV_8UC3, px.data());
        vector<cv::Mat> imgs = {img, cv::Mat(), img};
        const float thr = (float)atof(argv[8]);
        const vector<uint8_t> plain = det.detectFaceBatch(imgs, thr, spec);
        const vector<int> plain_off = det.faceBatchOffsets();
        const vector<uint8_t> tensor = det.detectFaceBatchGated(imgs, thr, spec, nullptr);
        if (tensor != plain || det.faceBatchOffsets() != plain_off) { fprintf(stderr, "the NULL gate changed the bytes\n"); return 3; }
        const int n = (int)imgs.size(), tr = det.faceBatchTruncated() ? 1 : 0, stride = det.faceBatchQualityStride();
        if ((int)det.faceBatchOffsets().size() != n + 1 || (int)det.lastBatchResult().size() != n ||
            det.faceBatchQuality().size() != (size_t)n * stride) { fprintf(stderr, "sizes disagree\n"); return 1; }
        FILE *out = fopen(argv[16], "wb");
        if (!out) return 2;
        fwrite(&n, sizeof(int), 1, out);
        fwrite(&tr, sizeof(int), 1, out);
        fwrite(det.faceBatchOffsets().data(), sizeof(int), (size_t)n + 1, out);
        for (const vector<FaceDetectInfo> &faces : det.lastBatchResult()) {
            const int k = (int)faces.size();
            fwrite(&k, sizeof(int), 1, out);
            fwrite(faces.data(), sizeof(FaceDetectInfo), k, out);
        }
        fwrite(&stride, sizeof(int), 1, out);
        fwrite(det.faceBatchQuality().data(), sizeof(rf_face_quality), (size_t)n * stride, out);
        const int got = (int)(det.faceBatchMatrices().size() / 6);
        fwrite(&got, sizeof(int), 1, out);
        fwrite(det.faceBatchMatrices().data(), sizeof(double), (size_t)got * 6, out);
        fwrite(tensor.data(), 1, tensor.size(), out);
        fclose(out);
        printf("faces %d of %d truncated %d bytes %zu\n", got, det.faceBatchOffsets()[n], tr, tensor.size());
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
