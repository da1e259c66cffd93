// TEST INFRASTRUCTURE ONLY: the command line of oracle/_ref/ref_host. It drives the reference's
// own compiled host code, taking the steps its renderer takes (Renderer.cc:157-217 and
// App.cc:166): importMesh -> Scene -> BVH(scene, Platform("GPU") with leaf preferences, params)
// -> CudaBVH(Compact2) -> serialize. Each subcommand writes raw bytes to a file and one JSON
// line to stdout; nothing here computes a compared value itself.
//
//   bvh OBJ OUT.dat [minLeaf maxLeaf splitAlpha]    defaults 1 8 1e-5
//   scene OBJ OUT.bin      the five Scene buffers in declaration order
//   reload IN.dat OUT.dat  CudaBVH(InputStream&), then serialize
//   hash FILE              hashBuffer over the file's bytes
//   pixeltable W H OUT.bin indexToPixel, then pixelToIndex
//   camera SIGNATURE       CameraControls::decodeSignature; every float as its bits
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "3d/CameraControls.hh"
#include "3d/Mesh.hh"
#include "base/Hash.hh"
#include "bvh/BVH.hh"
#include "cuda/CudaBVH.hh"
#include "io/File.hh"
#include "ray/PixelTable.hh"
#include "Scene.hh"

using namespace FW;

static void put(FILE* f, Buffer& b)
{
    if (b.getSize() && fwrite(b.getPtr(), 1, (size_t)b.getSize(), f) != (size_t)b.getSize())
    {
        fprintf(stderr, "ref_host: short write\n");
        exit(2);
    }
}

static FILE* create(const char* path)
{
    FILE* f = fopen(path, "wb");
    if (!f)
    {
        fprintf(stderr, "ref_host: cannot write %s\n", path);
        exit(2);
    }
    return f;
}

static Scene* loadScene(const char* obj)
{
    MeshBase* mesh = importMesh(obj);
    if (!mesh)
    {
        fprintf(stderr, "ref_host: cannot import %s\n", obj);
        exit(2);
    }
    return new Scene(*mesh);
}

static int cmdBvh(int argc, char** argv)
{
    int minLeaf = (argc > 4) ? atoi(argv[4]) : 1;
    int maxLeaf = (argc > 5) ? atoi(argv[5]) : 8;
    float alpha = (argc > 6) ? strtof(argv[6], NULL) : 1.0e-5f;

    Scene* scene = loadScene(argv[2]);
    Platform platform("GPU");
    platform.setLeafPreferences(minLeaf, maxLeaf);
    BVH::Stats stats;
    BVH::BuildParams params;
    params.stats = &stats;
    params.enablePrints = false;
    params.splitAlpha = alpha;
    BVHLayout layout = BVHLayout_Compact2;
    U32 sceneHash = scene->hash();
    U32 cache = hashBits(sceneHash, platform.computeHash(), params.computeHash(), layout);

    BVH bvh(scene, platform, params);
    CudaBVH cbvh(bvh, layout);
    {
        FileWR out(argv[3]);
        cbvh.serialize(out);
    }
    printf("{\"scene_hash\": \"%08x\", \"platform_hash\": \"%08x\", \"params_hash\": \"%08x\", "
           "\"cache_name\": \"%08x.dat\", \"num_triangles\": %d, \"num_vertices\": %d, "
           "\"nodes_bytes\": %lld, \"woop_bytes\": %lld, \"tri_index_bytes\": %lld, "
           "\"sah_cost_bits\": %u, \"branching_factor\": %d, \"num_inner_nodes\": %d, "
           "\"num_leaf_nodes\": %d, \"num_child_nodes\": %d, \"num_tris\": %d}\n",
           sceneHash, platform.computeHash(), params.computeHash(), cache,
           scene->getNumTriangles(), scene->getNumVertices(),
           (long long)cbvh.getNodeBuffer().getSize(), (long long)cbvh.getTriWoopBuffer().getSize(),
           (long long)cbvh.getTriIndexBuffer().getSize(),
           floatToBits(stats.SAHCost), stats.branchingFactor, stats.numInnerNodes, stats.numLeafNodes,
           stats.numChildNodes, stats.numTris);
    return 0;
}

static int cmdScene(char** argv)
{
    Scene* scene = loadScene(argv[2]);
    FILE* f = create(argv[3]);
    put(f, scene->getTriVtxIndexBuffer());
    put(f, scene->getTriNormalBuffer());
    put(f, scene->getTriMaterialColorBuffer());
    put(f, scene->getTriShadedColorBuffer());
    put(f, scene->getVtxPosBuffer());
    fclose(f);
    printf("{\"scene_hash\": \"%08x\", \"num_triangles\": %d, \"num_vertices\": %d}\n",
           scene->hash(), scene->getNumTriangles(), scene->getNumVertices());
    return 0;
}

static int cmdReload(char** argv)
{
    FileRO in(argv[2]);
    if (in.hasError())
    {
        fprintf(stderr, "ref_host: cannot read %s\n", argv[2]);
        return 2;
    }
    CudaBVH cbvh(in);
    {
        FileWR out(argv[3]);
        cbvh.serialize(out);
    }
    printf("{\"layout\": %d, \"nodes_bytes\": %lld, \"woop_bytes\": %lld, \"tri_index_bytes\": %lld}\n",
           (int)cbvh.getLayout(), (long long)cbvh.getNodeBuffer().getSize(),
           (long long)cbvh.getTriWoopBuffer().getSize(), (long long)cbvh.getTriIndexBuffer().getSize());
    return 0;
}

static int cmdHash(char** argv)
{
    FILE* f = fopen(argv[2], "rb");
    if (!f)
    {
        fprintf(stderr, "ref_host: cannot read %s\n", argv[2]);
        return 2;
    }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    char* data = (char*)malloc(n ? n : 1);
    if (fread(data, 1, n, f) != (size_t)n)
        return 2;
    fclose(f);
    U32 h = hashBuffer(data, (int)n);
    printf("{\"bytes\": %ld, \"hash_buffer\": \"%08x\", \"hash_bits_1\": \"%08x\", \"hash_bits_6\": \"%08x\"}\n",
           n, h, hashBits(h), hashBits(h, (U32)n, 1, 2, 3, 4));
    return 0;
}

static int cmdPixelTable(char** argv)
{
    PixelTable table;
    table.setSize(Vec2i(atoi(argv[2]), atoi(argv[3])));
    FILE* f = create(argv[4]);
    put(f, table.getIndexToPixel());
    put(f, table.getPixelToIndex());
    fclose(f);
    printf("{\"width\": %d, \"height\": %d}\n", table.getSize().x, table.getSize().y);
    return 0;
}

static int cmdCamera(char** argv)
{
    CameraControls camera;
    camera.decodeSignature(argv[2]);
    const Vec3f& p = camera.getPosition();
    const Vec3f& f = camera.getForward();
    const Vec3f& u = camera.getUp();
    printf("{\"position\": [%u, %u, %u], \"forward\": [%u, %u, %u], \"up\": [%u, %u, %u], "
           "\"fov\": %u, \"near\": %u, \"far\": %u, \"speed\": %u, \"keep_aligned\": %d}\n",
           floatToBits(p.x), floatToBits(p.y), floatToBits(p.z), floatToBits(f.x), floatToBits(f.y), floatToBits(f.z),
           floatToBits(u.x), floatToBits(u.y), floatToBits(u.z), floatToBits(camera.getFOV()),
           floatToBits(camera.getNear()), floatToBits(camera.getFar()), floatToBits(camera.getSpeed()),
           (int)camera.getKeepAligned());
    return 0;
}

int main(int argc, char** argv)
{
    const char* cmd = (argc > 1) ? argv[1] : "";
    if (!strcmp(cmd, "bvh") && argc >= 4)           return cmdBvh(argc, argv);
    if (!strcmp(cmd, "scene") && argc == 4)         return cmdScene(argv);
    if (!strcmp(cmd, "reload") && argc == 4)        return cmdReload(argv);
    if (!strcmp(cmd, "hash") && argc == 3)          return cmdHash(argv);
    if (!strcmp(cmd, "pixeltable") && argc == 5)    return cmdPixelTable(argv);
    if (!strcmp(cmd, "camera") && argc == 3)        return cmdCamera(argv);
    fprintf(stderr, "usage: ref_host bvh OBJ OUT.dat [minLeaf maxLeaf splitAlpha] | scene OBJ OUT.bin | "
                    "reload IN.dat OUT.dat | hash FILE | pixeltable W H OUT.bin | camera SIGNATURE\n");
    return 2;
}
